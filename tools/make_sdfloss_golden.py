"""Golden vectors of the mapper's SDF-sample loss block (utils/mapper.py:836-930) from the reference's own helpers.

`sdf_bce_loss` and `color_diff_loss` (utils/loss.py) and `Mapper.get_numerical_gradient` (utils/mapper.py:2319-2370,
called unbound on a stand-in whose `sdf` is the oracle's `mapper_sdf`) are imported from the reference tree; the map
query is the oracle's restatement (`oracle/sdf_cpu.NeuralPointMap.query_feature`, itself pinned by the `sdf_*.npz`
vectors) on the `sdf_gs_f32` and `sdf_pin_f8` maps in float64.  The inline lines of the SDF loop are transcribed below.
Writes tests/golden/sdfloss_*.npz with the inputs, the three terms, the subset sizes and the gradients of a weighted
sum; tests/test_sdf_losses.py reads only the files.

    python tools/make_sdfloss_golden.py            (needs the reference tree; CPU only)
"""
import sys
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from oracle import ref_shim, sdf_cpu  # noqa: E402


def helpers():
    ref_shim.load()                      # stubs the reference's non-arithmetic imports, puts the tree on sys.path
    from utils.loss import color_diff_loss, sdf_bce_loss  # type: ignore
    from unittest.mock import MagicMock

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
    return sdf_bce_loss, color_diff_loss, Mapper.get_numerical_gradient


def block(H, cfg, sdf_scale, npm, dec, cmlp, coord, sdf_label, ts, weight, color_label, color_weighted):
    """utils/mapper.py:836-930 with BCE, the numerical Eikonal term and the colour term on (un-weighted terms)."""
    sdf_bce_loss, color_diff_loss, get_numerical_gradient = H
    valid_color_mask = (torch.abs(sdf_label) < 0.5 * cfg.surface_sample_range_m) & (color_label[:, 0] >= 0.0)
    apply_eikonal_mask = (torch.abs(sdf_label) < cfg.free_sample_end_dist_m)
    geo_feature, color_feature, weight_knn, _, certainty = npm.query_feature(coord, ts, query_color_feature=True)
    sdf_pred = dec.sdf(geo_feature)
    if not cfg.weighted_first:
        sdf_pred = torch.sum(sdf_pred * weight_knn, dim=1).squeeze(1)
    color_pred = torch.sigmoid(cmlp.mlp(color_feature[valid_color_mask]))     # Decoder.regress_color
    if not cfg.weighted_first:
        color_pred = torch.sum(color_pred * weight_knn[valid_color_mask], dim=1)
    coord_for_eikonal = coord[apply_eikonal_mask]
    sdf_pred_for_eikonal = sdf_pred[apply_eikonal_mask]
    this = NS(sdf=lambda x: (sdf_cpu.mapper_sdf(npm, dec, x)[0], None, None))
    g = get_numerical_gradient(this, coord_for_eikonal[::cfg.gradient_decimation],
                               sdf_pred_for_eikonal[::cfg.gradient_decimation],
                               cfg.voxel_size_m * cfg.num_grad_step_ratio)
    weight = torch.abs(weight).detach()
    sdf_loss = sdf_bce_loss(sdf_pred, sdf_label, sdf_scale, weight, cfg.loss_weight_on)
    eikonal_loss = ((g.norm(2, dim=-1) - 1.0) ** 2).mean()
    color_loss = color_diff_loss(color_pred, color_label[valid_color_mask], weight[valid_color_mask], color_weighted,
                                 l2_loss=False)
    return [sdf_loss, eikonal_loss, color_loss], [int(g.shape[0]), int(valid_color_mask.sum())]


def main():
    from test_sdf_losses import (GOLDEN_CASES, LOSS_W, _batch, _cfg, _cmlp_params, _dec_params, _sigma, _state)

    import sdf_losses_ref as ref

    H = helpers()
    out_dir = ROOT / "tests" / "golden"
    for name, c in GOLDEN_CASES.items():
        st = _state(name)
        cfg = _cfg(st, d=c["d"], loss_weight_on=c["loss_weight_on"])
        coord, label, ts, weight, color_label = _batch(st, B=400, seed=11)
        cm_p = _cmlp_params(st, seed=12)
        geo = torch.as_tensor(st["local_geo_features"]).double().requires_grad_(True)
        col = torch.as_tensor(st["local_color_features"]).double().requires_grad_(True)
        p64 = [p.double().requires_grad_(True) for p in _dec_params(st) + cm_p]
        npm = ref.map64(st, geo, col)
        dec = sdf_cpu.MLP(*p64[:4], float(st["sdf_scale"]))
        cm = sdf_cpu.MLP(*p64[4:])
        vals, counts = block(H, cfg, _sigma(st), npm, dec, cm, coord.double(), label.double(), ts, weight.double(),
                             color_label.double(), c["color_weighted"])
        tot = sum(w * v for w, v in zip(LOSS_W, vals))
        grads = torch.autograd.grad(tot, [geo, col] + p64)
        rec = {"coord": coord.numpy(), "label": label.numpy(), "ts": ts.numpy(), "weight": weight.numpy(),
               "color_label": color_label.numpy(), "values": np.array([float(v.detach()) for v in vals]),
               "counts": np.array(counts), "weights": np.array(LOSS_W)}
        for k, p in zip(("W1", "b1", "W2", "b2"), cm_p):
            rec["cmlp." + k] = p.numpy()
        for k, g in zip(["local_geo_features", "local_color_features", "dec.W1", "dec.b1", "dec.W2", "dec.b2",
                         "color.W1", "color.b1", "color.W2", "color.b2"], grads):
            rec["d_" + k] = g.numpy()
        np.savez_compressed(out_dir / f"sdfloss_{name}.npz", **rec)
        print(name, [round(float(v), 6) for v in vals], counts)


if __name__ == "__main__":
    main()
