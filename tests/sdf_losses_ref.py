"""fp64 restatement of the mapper's SDF-sample loss block (utils/mapper.py:836-930 and 1493-1544; the BCE and colour
helpers of utils/loss.py:30-63) for the tests of `pings_amd.sdf_losses`, over the oracle's
`NeuralPointMap.query_feature` and `MLP` (oracle/sdf_cpu.py).  The inline lines are transcribed term for term; the
reference's own helpers pin this file through tests/golden/sdfloss_*.npz (tools/make_sdfloss_golden.py)."""
import torch

from oracle import sdf_cpu


def color_diff_loss(pred, label, weight=1.0, weighted=False):                   # utils/loss.py:30-40 (L1)
    w = weight.unsqueeze(1) if weighted else 1.0
    return (w * torch.abs(pred - label)).mean()


def sdf_bce_loss(pred, label, sigma, weight, weighted=False):                  # utils/loss.py:45-63
    bce = torch.nn.BCEWithLogitsLoss(reduction="mean", weight=weight if weighted else None)
    return bce(pred / sigma, torch.sigmoid(label / sigma))


def numerical_gradient(sdf, x, eps):                                           # utils/mapper.py:2319-2348
    N = x.shape[0]
    e = torch.eye(3, dtype=x.dtype) * eps
    xs = torch.cat((x + e[0], x - e[0], x + e[1], x - e[1], x + e[2], x - e[2]), dim=0)
    s = sdf(xs).unsqueeze(-1)
    return torch.cat([(s[:N] - s[N:2 * N]) / (2 * eps), (s[2 * N:3 * N] - s[3 * N:4 * N]) / (2 * eps),
                      (s[4 * N:5 * N] - s[5 * N:]) / (2 * eps)], dim=1)


def block(cfg, sdf_scale, npm, dec, cmlp, coord, sdf_label, ts, weight, color_label=None, eikonal=True, color=False,
          color_weighted=False):
    """Returns (bce, eikonal, colour, eikonal rows, colour rows, sdf_pred); a disabled term is 0.0.
    `npm` is an `sdf_cpu.NeuralPointMap` (float64 tensors), `dec` / `cmlp` `sdf_cpu.MLP`s."""
    wf = npm.weighted_first
    valid_color_mask = None
    if color:
        valid_color_mask = (torch.abs(sdf_label) < 0.5 * cfg.surface_sample_range_m) & (color_label[:, 0] >= 0.0)
    apply_eikonal_mask = torch.abs(sdf_label) < cfg.free_sample_end_dist_m
    geo_feature, color_feature, weight_knn, _, _ = npm.query_feature(coord, ts, query_color_feature=color)
    sdf_pred = dec.sdf(geo_feature)
    if not wf:
        sdf_pred = torch.sum(sdf_pred * weight_knn, dim=1).squeeze(1)
    color_pred = None
    if color:
        color_pred = torch.sigmoid(cmlp.mlp(color_feature[valid_color_mask]))      # Decoder.regress_color
        if not wf:
            color_pred = torch.sum(color_pred * weight_knn[valid_color_mask], dim=1)
    weight = torch.abs(weight).detach()
    bce = sdf_bce_loss(sdf_pred, sdf_label, sdf_scale, weight, cfg.loss_weight_on)
    eik, n_eik = 0.0, 0
    if eikonal:
        x = coord[apply_eikonal_mask][::cfg.gradient_decimation]
        n_eik = x.shape[0]

        def sdf(q):                                  # Mapper.sdf (mapper.py:2273-2289), no certainty side effects
            return sdf_cpu.mapper_sdf(npm, dec, q)[0]
        g = numerical_gradient(sdf, x, cfg.voxel_size_m * cfg.num_grad_step_ratio)
        eik = ((g.norm(2, dim=-1) - 1.0) ** 2).mean()
    col, n_col = 0.0, 0
    if color:
        n_col = int(valid_color_mask.sum())
        col = color_diff_loss(color_pred, color_label[valid_color_mask], weight[valid_color_mask], color_weighted)
    return bce, eik, col, n_eik, n_col, sdf_pred


def map64(st, geo=None, col=None):
    """The oracle map of a golden state in float64; `geo` / `col` replace the local feature tables (leaves)."""
    npm = sdf_cpu.NeuralPointMap(st)
    for k, v in list(vars(npm).items()):
        if torch.is_tensor(v) and v.dtype == torch.float32:
            setattr(npm, k, v.double())
    npm.dtype = torch.float64
    if geo is not None:
        npm.local_geo_features = geo
    if col is not None:
        npm.local_color_features = col
    return npm
