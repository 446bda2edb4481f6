"""Golden vectors of the mapper's per-frame point tests from the reference's own functions.

`Mapper.dynamic_filter`, `Mapper.dynamic_filter_neural_points` and `Mapper.check_invalid_neural_points`
(utils/mapper.py:528-585, :1636-1655) are called unbound on stand-ins whose `neural_points` is the reference's own
`NeuralPoints` (the maps of tests/golden/sdf_*.npz, rebuilt by oracle/make_golden.py's recipe) and whose `sdf_mlp` is its
`Decoder`.  The new-sample block of `process_frame` (:447-513) is cut out of the method's source at run time and run on
the same stand-ins.  Writes tests/golden/frame_*.npz (inputs, config scalars, outputs); tests/test_frame_ops.py reads
only the files.

    python tools/make_frame_golden.py            (needs the reference tree; CPU only)
"""
import inspect
import sys
import textwrap
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

from make_pool_golden import reference  # noqa: E402
from oracle import make_golden as MG  # noqa: E402

SCALARS = ("voxel_size_m", "new_certainty_thre", "surface_sample_range_m", "dynamic_certainty_thre",
           "dynamic_sdf_ratio_thre", "dynamic_min_grad_norm_thre", "infer_bs", "adaptive_iters", "new_sample_ratio_less",
           "new_sample_ratio_more", "new_sample_ratio_restart", "freeze_after_frame", "bs_new_sample")


def new_sample_block(Mapper):
    """`def block(self, frame_id)` holding lines :447-513 of `process_frame`, compiled in the module of `Mapper`."""
    lines = inspect.getsource(Mapper.process_frame).splitlines()
    first = next(i for i, l in enumerate(lines) if l.strip() == "if (" and "bs_new_sample > 0" in lines[i + 1])
    last = next(i for i in range(first, len(lines)) if lines[i].strip().startswith("T3_3 = get_time()"))
    body = textwrap.dedent("\n".join(lines[first:last]))
    src = "def block(self, frame_id):\n" + textwrap.indent(body, "    ") + "\n"
    scope = dict(vars(sys.modules[Mapper.__module__]))
    exec(compile(src, "process_frame[447:513]", "exec"), scope)
    return scope["block"]


def main():
    import frame_ref as FR

    R, _, Mapper = reference()
    block = new_sample_block(Mapper)
    out_dir = ROOT / "tests" / "golden"
    for case in FR.CASES:
        st = FR.load_state(out_dir, case)
        cfg, npm = MG.build_reference_map(R, MG.SDF_CASES[case], seed=len(case))
        gen = torch.Generator().manual_seed(99)
        dec = R.Decoder(cfg, cfg.feature_dim, cfg.geo_mlp_hidden_dim, cfg.geo_mlp_level, 1)
        with torch.no_grad():
            for p in dec.parameters():
                p.copy_(torch.randn(p.shape, generator=gen) * 0.3)
        # the map and the decoder are the ones the SDF fixtures hold
        assert torch.equal(npm.neural_points, torch.as_tensor(st["neural_points"]))
        assert torch.equal(npm.local_geo_features.detach(), torch.as_tensor(st["local_geo_features"]))
        assert torch.equal(npm.buffer_pt_index[torch.as_tensor(st["table_slots"])], torch.as_tensor(st["table_vals"]))
        assert torch.equal(dec.layers[0].weight.detach(), torch.as_tensor(st["dec.layers.0.weight"]))
        assert torch.equal(dec.lout.bias.detach(), torch.as_tensor(st["dec.lout.bias"]))
        for k, v in vars(FR.make_config(case, st)).items():
            setattr(cfg, k, v)
        cert_global, cert_local = FR.certainty_tables(st)
        npm.point_certainties = cert_global.clone()
        npm.local_point_certainties = cert_local.clone()
        rec = {"cert_global": cert_global.numpy(), "cert_local": cert_local.numpy()}
        for k in SCALARS:
            rec["cfg_" + k] = np.asarray(getattr(cfg, k))
        rec["cfg_check_ratio"] = np.asarray(FR.CHECK_RATIO[case])

        # ---- new samples
        coord, label = FR.frame_samples(st, FR.FIXTURE_ROWS, seed=21)
        rec["new_coord"], rec["new_label"], rec["new_history"] = coord.numpy(), label.numpy(), np.asarray(FR.HISTORY)
        dx_before = npm.neighbor_dx.clone()
        for frame_id in (0, 31):
            m = types.SimpleNamespace(config=cfg, neural_points=npm, device=torch.device("cpu"), silence=True,
                                      **FR.pool_of(coord, label, FR.HISTORY))
            block(m, frame_id)
            rec[f"o_new_idx_f{frame_id}"] = m.new_idx.numpy()
            rec[f"o_new_obs_ratio_f{frame_id}"] = np.asarray(m.new_obs_ratio)
            rec[f"o_adaptive_iter_offset_f{frame_id}"] = np.asarray(m.adaptive_iter_offset)
        assert torch.equal(npm.neighbor_dx, dx_before)      # the "dirty fix" put the neighbourhood back
        print(case, "new samples", m.new_idx.shape[0], "of", FR.FIXTURE_ROWS, "ratio", m.new_obs_ratio,
              "offsets", rec["o_adaptive_iter_offset_f0"], rec["o_adaptive_iter_offset_f31"])

        # ---- dynamic filters
        x = FR.frame_points(st, FR.FIXTURE_ROWS, seed=11)
        rec["dyn_points"] = x.numpy()
        m = types.SimpleNamespace(config=cfg, neural_points=npm, sdf_mlp=dec, device=torch.device("cpu"),
                                  dtype=torch.float32, silence=True)
        for on in (True, False):
            rec[f"o_static_type2_{int(on)}"] = Mapper.dynamic_filter(m, x.clone(), on).numpy()
        rec["o_static_neural_points"] = Mapper.dynamic_filter_neural_points(m).detach().numpy()
        print(case, "static", [float(rec[k].mean()) for k in ("o_static_type2_1", "o_static_type2_0",
                                                                "o_static_neural_points")])

        # ---- check_invalid_neural_points
        m.sdf = types.MethodType(Mapper.sdf, m)
        m.sdf_batch = types.MethodType(Mapper.sdf_batch, m)
        cfg.dynamic_sdf_ratio_thre = FR.CHECK_RATIO[case]
        lv0, gv0 = npm.local_valid_gs_mask.clone(), npm.valid_gs_mask.clone()
        assert torch.equal(lv0, torch.as_tensor(st["local_valid_gs_mask"]))
        for min_nn in FR.CHECK_MIN_NN:
            npm.local_valid_gs_mask, npm.valid_gs_mask = lv0.clone(), gv0.clone()
            Mapper.check_invalid_neural_points(m, FR.STABILITY_THRESHOLD, min_nn)
            rec[f"o_local_valid_nn{min_nn}"] = npm.local_valid_gs_mask.numpy().copy()
            rec[f"o_valid_nn{min_nn}"] = npm.valid_gs_mask.numpy().copy()
            print(case, "valid, min_nn", min_nn, int(npm.local_valid_gs_mask.sum()), "of", lv0.numel(),
                  "before", int(lv0.sum()))
        np.savez_compressed(out_dir / f"frame_{case}.npz", **rec)


if __name__ == "__main__":
    main()
