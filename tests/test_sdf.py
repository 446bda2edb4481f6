"""Neural-point SDF query: oracle vs the reference's golden vectors (CPU), HIP vs oracle (GPU)."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import mlp_ref
from conftest import rel_err
from oracle import sdf_cpu

CASES = ["gs_f32", "pin_f8", "pgo_f32"]

# pings_sdf_plan (csrc/sdf_plan.hpp): kernel family, order of differentiation
VECTOR, MATRIX = 0, 1
FWD, BWD, BWD2 = 0, 1, 2


def _plan(nn_k, F, H, weighted_first=False, order=FWD, misaligned=False):
    """(family, IN_PAD class) of the kernel the library runs for this shape and order; needs no GPU."""
    from pings_amd import _lib

    out = (ctypes.c_int32 * 2)()
    assert _lib.lib().pings_sdf_plan(nn_k, F, H, int(weighted_first), order, int(misaligned), out) == 0
    return out[0], out[1]


def load(golden_dir, name):
    z = np.load(golden_dir / f"sdf_{name}.npz")
    return {k: z[k] for k in z.files}


def T(a):
    return torch.from_numpy(np.asarray(a))


# ------------------------------------------------------------------ CPU: oracle pinned by the reference
@pytest.mark.parametrize("name", CASES)
def test_oracle_radius_search_matches_reference(golden_dir, name):
    st = load(golden_dir, name)
    npm = sdf_cpu.NeuralPointMap(st)
    assert torch.equal(npm.neighbor_dx, sdf_cpu.neighbor_offsets(2, {"gs_f32": 0.8, "pin_f8": 0.5, "pgo_f32": 0.8}[name]))
    for tf in (0, 1):
        d2, idx = npm.radius_neighborhood_search(T(st["x"]), time_filtering=bool(tf))
        assert torch.equal(idx, T(st[f"g1_idx_tf{tf}"]))          # index-exact
        assert torch.equal(d2, T(st[f"g1_d2_tf{tf}"]))            # same op sequence -> bit-exact on CPU


@pytest.mark.parametrize("name", CASES)
def test_oracle_query_feature_matches_reference(golden_dir, name):
    st = load(golden_dir, name)
    npm = sdf_cpu.NeuralPointMap(st)
    x = T(st["x"])
    qts = torch.full((x.shape[0],), 2, dtype=torch.int32)
    geo, col, w, cnt, cert = npm.query_feature(x, qts, accumulate_stability=True, query_locally=True,
                                               query_color_feature=True)
    assert torch.equal(cnt, T(st["g2_cnt"]))
    for a, k in ((geo, "g2_geo"), (col, "g2_color"), (w, "g2_w"), (cert, "g2_cert")):
        assert rel_err(a, T(st[k])) <= 1e-6, k
    assert rel_err(npm.local_point_certainties, T(st["g2_local_cert_after"])) <= 1e-6
    assert torch.equal(npm.local_point_ts_update, T(st["g2_local_ts_after"]))
    npm = sdf_cpu.NeuralPointMap(st)
    geo, _, w, cnt, cert = npm.query_feature(x, None, accumulate_stability=False, query_locally=False,
                                             use_only_valid_points=True)
    assert torch.equal(cnt, T(st["g2_cnt_global"]))
    assert rel_err(geo, T(st["g2_geo_global"])) <= 1e-6 and rel_err(w, T(st["g2_w_global"])) <= 1e-6
    assert rel_err(cert, T(st["g2_cert_global"])) <= 1e-6


@pytest.mark.parametrize("name", CASES)
def test_oracle_sdf_gradient_and_double_backward_match_reference(golden_dir, name):
    st = load(golden_dir, name)
    npm = sdf_cpu.NeuralPointMap(st)
    dec = sdf_cpu.MLP.from_state(st)
    npm.local_geo_features.requires_grad_(True)
    for p in dec.parameters():
        p.requires_grad_(True)
    x = T(st["x"]).clone().requires_grad_(True)
    s, cnt = sdf_cpu.mapper_sdf(npm, dec, x)
    g = sdf_cpu.get_gradient(x, s)
    loss = ((g.norm(dim=-1) - 1.0) ** 2).mean() + s.abs().mean()
    grads = torch.autograd.grad(loss, [npm.local_geo_features] + dec.parameters())
    assert rel_err(s, T(st["g3_sdf"])) <= 1e-5
    assert rel_err(g, T(st["g3_grad_x"])) <= 1e-5
    assert abs(loss.item() - float(st["g3_loss"])) <= 1e-5
    assert rel_err(grads[0], T(st["g3_dfeat"])) <= 1e-4
    for gk, k in zip(grads[1:], ["layers.0.weight", "layers.0.bias", "lout.weight", "lout.bias"]):
        assert rel_err(gk, T(st["g3_d." + k])) <= 1e-4, k


def test_synthetic_map_follows_the_reference_hash_rule():
    st, dec = sdf_cpu.synthetic_map(3000, buffer_size=20011)   # small table -> collisions
    npm = sdf_cpu.NeuralPointMap({**st})
    pts = npm.neural_points
    cells = torch.floor(pts / npm.resolution).to(torch.int64)
    h = torch.fmod((cells * npm.primes).sum(-1), npm.buffer_size)
    got = npm.buffer_pt_index[h]            # python-style negative wrap, like the reference
    # every point finds a point in ITS slot; where no collision happened it finds itself
    assert (got >= 0).all()
    assert (got == torch.arange(pts.shape[0])).float().mean() > 0.8
    x = sdf_cpu.synthetic_queries(st, 500)
    s, cnt = sdf_cpu.mapper_sdf(npm, sdf_cpu.MLP.from_state({**dec}), x)
    assert (cnt > 0).float().mean() > 0.9 and torch.isfinite(s).all()


# ------------------------------------------------------------------ GPU: HIP vs golden / oracle
def _gpu_map(st):
    """The oracle's plain-tensor map moved to the device, dressed with the few config attributes the
    reference's NeuralPoints carries, so the HIP `query_feature` can be bound to it like to the real class."""
    from types import SimpleNamespace

    npm = sdf_cpu.NeuralPointMap(st, device="cuda")
    npm.config = SimpleNamespace(query_nn_k=npm.nn_k, weighted_first=npm.weighted_first, layer_norm_on=False)
    npm.color_feature_dim = npm.color_features.shape[1] if npm.color_features is not None else 0
    return npm


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_topk_is_index_exact(golden_dir, name):
    from pings_amd import neural_points as hnp

    st = load(golden_dir, name)
    cpu = sdf_cpu.NeuralPointMap(st)
    gpu = _gpu_map(st)
    x = T(st["x"])
    for local, meas, val in [(True, True, False), (False, True, True), (False, False, False), (True, False, True)]:
        ri, rd, rc = cpu.search_topk(x, query_locally=local, use_only_measured_points=meas,
                                     use_only_valid_points=val)
        hi, hd, hc = hnp.radius_neighborhood_topk(gpu, x.cuda(), time_filtering=cpu.temporal_local_map_on and local,
                                                  use_only_measured_points=meas, use_only_valid_points=val,
                                                  query_locally=local)
        assert torch.equal(hc.cpu(), rc)
        assert torch.equal(hi.cpu(), ri)        # bit-exact neighbour indices and order
        assert torch.equal(hd.cpu(), rd)        # bit-exact fp32 squared distances


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_radius_search_matches_reference_golden(golden_dir, name):
    """`radius_neighborhood_search` as it stands (model/neural_gaussians.py:1061-1115) against the reference's own
    outputs (G1): every candidate cell's index and squared distance bit for bit, with and without the travel-distance
    window; then `query_certainty` (:1117-1133) on top of it with the mapper's one-cell neighbourhood
    (utils/mapper.py:461-475) against the oracle."""
    from pings_amd import neural_points as hnp

    st = load(golden_dir, name)
    gpu = _gpu_map(st)
    x = T(st["x"])
    for tf in (0, 1):
        d2, idx = hnp.radius_neighborhood_search(gpu, x.cuda(), time_filtering=bool(tf))
        assert torch.equal(idx.cpu(), T(st[f"g1_idx_tf{tf}"]))
        assert torch.equal(d2.cpu(), T(st[f"g1_d2_tf{tf}"]))
    cpu = sdf_cpu.NeuralPointMap(st)
    one_cell = sdf_cpu.neighbor_offsets(1, 0.0)
    assert one_cell.shape[0] == 1
    for m_ in (cpu, gpu):
        m_.neighbor_dx = one_cell.to(m_.neural_points.device)
        m_.max_valid_dist2 = 3 * ((1 + 1) * m_.resolution) ** 2

    def certainty(m_, search, pts):   # the reference's query_certainty, line by line
        _, i = search(pts)
        c = m_.point_certainties[i]
        c[i < 0] = 0.0
        return torch.max(c, dim=-1)[0]

    ref = certainty(cpu, cpu.radius_neighborhood_search, x)
    got = certainty(gpu, lambda p: hnp.radius_neighborhood_search(gpu, p), x.cuda())
    assert torch.equal(got.cpu(), ref) and float(ref.max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_query_feature_matches_reference_golden(golden_dir, name):
    from pings_amd import neural_points as hnp

    st = load(golden_dir, name)
    npm = _gpu_map(st)
    x = T(st["x"]).cuda()
    qts = torch.full((x.shape[0],), 2, dtype=torch.int32, device="cuda")
    geo, col, w, cnt, cert = hnp.query_feature(npm, x, qts, accumulate_stability=True, query_locally=True,
                                               query_color_feature=True)
    assert torch.equal(cnt.cpu(), T(st["g2_cnt"]))
    for a, k in ((geo, "g2_geo"), (col, "g2_color"), (w, "g2_w"), (cert, "g2_cert")):
        assert rel_err(a, T(st[k])) <= 1e-5, k
    assert rel_err(npm.local_point_certainties, T(st["g2_local_cert_after"])) <= 1e-5
    assert torch.equal(npm.local_point_ts_update.cpu(), T(st["g2_local_ts_after"]))
    npm = _gpu_map(st)
    geo, _, w, cnt, cert = hnp.query_feature(npm, x, None, accumulate_stability=False, query_locally=False,
                                             use_only_valid_points=True)
    assert torch.equal(cnt.cpu(), T(st["g2_cnt_global"]))
    assert rel_err(geo, T(st["g2_geo_global"])) <= 1e-5 and rel_err(w, T(st["g2_w_global"])) <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_sdf_autograd_and_double_backward_match_reference_golden(golden_dir, name):
    from pings_amd import neural_points as hnp

    st = load(golden_dir, name)
    npm = _gpu_map(st)
    dec = sdf_cpu.MLP.from_state(st, device="cuda")
    npm.local_geo_features.requires_grad_(True)
    for p in dec.parameters():
        p.requires_grad_(True)
    x = T(st["x"]).cuda().requires_grad_(True)
    geo, _, w, cnt, _ = hnp.query_feature(npm, x, accumulate_stability=False)
    s = dec.sdf(geo)
    if not npm.weighted_first:
        s = torch.sum(s * w, dim=1).squeeze(1)
    g = sdf_cpu.get_gradient(x, s)
    loss = ((g.norm(dim=-1) - 1.0) ** 2).mean() + s.abs().mean()
    grads = torch.autograd.grad(loss, [npm.local_geo_features] + dec.parameters())
    assert rel_err(s, T(st["g3_sdf"])) <= 1e-4
    assert rel_err(g, T(st["g3_grad_x"])) <= 1e-4
    assert rel_err(grads[0], T(st["g3_dfeat"])) <= 1e-4
    for gk, k in zip(grads[1:], ["layers.0.weight", "layers.0.bias", "lout.weight", "lout.bias"]):
        assert rel_err(gk, T(st["g3_d." + k])) <= 1e-4, k


class _Dec:
    """Duck-typed `Decoder` (model/decoder.py) built from the fixture's state dict."""

    def __init__(self, st, device="cuda"):
        from types import SimpleNamespace as NS

        t = lambda k: T(st["dec." + k]).to(device)
        self.layers = [NS(weight=t("layers.0.weight"), bias=t("layers.0.bias"))]
        self.lout = NS(weight=t("lout.weight"), bias=t("lout.bias"))
        self.sdf_scale = float(st["sdf_scale"])
        self.use_leaky_relu = False


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_fused_sdf_vector_and_matrix_core_kernels_agree(golden_dir, name, monkeypatch):
    """`pings_sdf_forward` has two kernels (csrc/knn_sdf.hip lane-per-hidden-unit, csrc/sdf_fwd_mfma.hip four queries
    per wave on the matrix cores); PINGS_SDF_FWD=vector forces the first.  Same neighbours, weights and counts bit for
    bit; SDF, gradient and spread within fp32 summation-order noise of each other (and each within 1e-4 of the
    reference: the golden test below runs the default, this one checks the forced kernel too)."""
    from pings_amd import neural_points as hnp

    st = load(golden_dir, name)
    gpu = _gpu_map(st)
    x = T(st["x"]).cuda()
    dec = _Dec(st)
    # the comparison means something only where the default plan is the matrix-core kernel: pin_f8 is weighted_first
    # and plans the vector kernel either way
    monkeypatch.delenv("PINGS_SDF_FWD", raising=False)
    F, H = gpu.local_geo_features.shape[1], dec.layers[0].weight.shape[0]
    assert gpu.local_geo_features.data_ptr() % 16 == 0
    want = {"gs_f32": (MATRIX, 36), "pin_f8": (VECTOR, 12), "pgo_f32": (MATRIX, 36)}[name]
    assert _plan(gpu.nn_k, F, H, gpu.weighted_first, FWD) == want
    out = {}
    for mode in ("mfma", "vector"):
        monkeypatch.setenv("PINGS_SDF_FWD", mode)
        assert _plan(gpu.nn_k, F, H, gpu.weighted_first, FWD)[0] == (want[0] if mode == "mfma" else VECTOR)
        out[mode] = hnp.sdf_fused(gpu, dec, x, need_grad=True, need_certainty=True, need_std=True)
    for a, b in zip(out["mfma"], out["vector"]):
        if a.dtype == torch.int64:
            assert torch.equal(a, b)
        else:
            assert rel_err(a, b) <= 2e-5, rel_err(a, b)
    if "g3_sdf" in st and not gpu.weighted_first:
        assert rel_err(out["vector"][0], T(st["g3_sdf"])) <= 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_fused_sdf_matches_reference_golden(golden_dir, name):
    from pings_amd import neural_points as hnp

    st = load(golden_dir, name)
    npm = _gpu_map(st)
    x = T(st["x"]).cuda()
    sdf, grad, cnt, cert = hnp.sdf_fused(npm, _Dec(st), x, need_grad=True, need_certainty=True)
    cpu = sdf_cpu.NeuralPointMap(st)
    _, _, rc = cpu.search_topk(T(st["x"]))
    assert torch.equal(cnt.cpu(), rc)
    assert rel_err(sdf, T(st["g3_sdf"])) <= 1e-4          # tolerance: north_star 1e-4 rel
    assert rel_err(grad, T(st["g3_grad_x"])) <= 1e-4
    # rows without any neighbour: exactly 0 (per-neighbour mode) or MLP(0)*scale (weighted-first)
    zero = (cnt == 0)
    assert zero.any()
    if not npm.weighted_first:
        assert (sdf[zero] == 0).all()
    assert (grad[zero] == 0).all()
    _, _, _, _, rcert = cpu.query_feature(T(st["x"]), accumulate_stability=False)
    assert rel_err(cert, rcert) <= 1e-5


@pytest.mark.gpu
def test_hip_fused_sdf_large_map_against_oracle():
    """SURVEY.md §8d Metric-2 shape (1e6 neural points, 1e8-slot table): 4096 queries vs the CPU oracle."""
    from pings_amd import neural_points as hnp

    st, dec = sdf_cpu.synthetic_map(1_000_000)
    x = sdf_cpu.synthetic_queries(st, 4096)
    cpu = sdf_cpu.NeuralPointMap({**st})
    ri, rd, rc = cpu.search_topk(x, use_only_measured_points=False)
    s_ref, _ = sdf_cpu.mapper_sdf(cpu, sdf_cpu.MLP.from_state({**dec}), x)
    gpu = _gpu_map({**st})
    hi, hd, hc = hnp.radius_neighborhood_topk(gpu, x.cuda(), query_locally=True)
    assert torch.equal(hi.cpu(), ri) and torch.equal(hc.cpu(), rc) and torch.equal(hd.cpu(), rd)
    sdf, _, cnt, _ = hnp.sdf_fused(gpu, _Dec({**dec}), x.cuda(), use_only_measured_points=False)
    assert rel_err(sdf, s_ref) <= 1e-4
    # empty batch
    e, _, c, _ = hnp.sdf_fused(gpu, _Dec({**dec}), x[:0].cuda())
    assert e.numel() == 0 and c.numel() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("kernel", ["mfma", "vector"])
def test_hip_fused_sdf_backward_matches_oracle_autograd(golden_dir, name, kernel, monkeypatch):
    """First-order training gradients (features + decoder) of the fused kernel vs autograd through the oracle
    (itself pinned to the reference by G1-G3), for both gradient kernels of `pings_sdf_backward` (csrc/sdf_bwd.hip:
    the matrix-core one is the default where it applies, PINGS_SDF_BWD=vector forces the lane-per-hidden-unit one)."""
    from types import SimpleNamespace as NS

    from pings_amd import neural_points as hnp

    monkeypatch.setenv("PINGS_SDF_BWD", kernel)
    st = load(golden_dir, name)
    x = T(st["x"])
    cpu = sdf_cpu.NeuralPointMap(st)
    dec_c = sdf_cpu.MLP.from_state(st)
    cpu.local_geo_features.requires_grad_(True)
    for p in dec_c.parameters():
        p.requires_grad_(True)
    s_ref, _ = sdf_cpu.mapper_sdf(cpu, dec_c, x)
    gw = torch.randn(x.shape[0], generator=torch.Generator().manual_seed(3))
    ref = torch.autograd.grad((s_ref * gw).sum(), [cpu.local_geo_features] + dec_c.parameters())

    gpu = _gpu_map(st)
    gpu.local_geo_features.requires_grad_(True)
    t = lambda k: torch.nn.Parameter(T(st["dec." + k]).cuda())
    d = NS(layers=[NS(weight=t("layers.0.weight"), bias=t("layers.0.bias"))],
           lout=NS(weight=t("lout.weight"), bias=t("lout.bias")), sdf_scale=float(st["sdf_scale"]), use_leaky_relu=False)
    outs = []
    for _ in range(2):
        sdf, cnt = hnp.sdf_train(gpu, d, x.cuda())
        got = torch.autograd.grad((sdf * gw.cuda()).sum(),
                                  [gpu.local_geo_features, d.layers[0].weight, d.layers[0].bias, d.lout.weight, d.lout.bias])
        outs.append(got)
    assert rel_err(sdf, s_ref) <= 1e-4
    for a, b, nm in zip(outs[0], ref, ["features", "W1", "b1", "W2", "b2"]):
        assert rel_err(a.reshape(b.shape), b) <= 1e-4, nm          # tolerance: north_star 1e-4 rel
    for a, b in zip(*outs):
        assert torch.equal(a, b)                                   # bitwise reproducible scatter


# ------------------------------------------------------------------ HIP map update followed by HIP queries
def _dress_map(m, nn_k=6, search_alpha=0.8):
    """Give a `neural_map.new_map` attribute bag the query-side attributes of the reference's NeuralPoints."""
    from types import SimpleNamespace

    dev = m.neural_points.device
    m.neighbor_dx = sdf_cpu.neighbor_offsets(2, search_alpha).to(dev)
    m.max_valid_dist2 = 3 * ((2 + 1) * m.resolution) ** 2
    m.after_pgo = False
    m.nn_k = nn_k
    m.weighted_first = False
    m.dtype = torch.float32
    m.config = SimpleNamespace(query_nn_k=nn_k, weighted_first=False, layer_norm_on=False, use_mid_ts=m.use_mid_ts,
                               range_filter_2d=m.range_filter_2d, local_map_radius=m.local_map_radius)
    return m


def _state_of(m):
    """CPU state dict of a HIP map for oracle/sdf_cpu.NeuralPointMap."""
    c = lambda t: t.detach().cpu().numpy()
    return dict(buffer_size=int(m.buffer_size), buffer_pt_index=c(m.buffer_pt_index), neural_points=c(m.neural_points),
                point_orientations=c(m.point_orientations), geo_features=c(m.geo_features),
                point_ts_create=c(m.point_ts_create), point_certainties=c(m.point_certainties),
                free_gs_mask=c(m.free_gs_mask), valid_gs_mask=c(m.valid_gs_mask), travel_dist=c(m.travel_dist),
                cur_ts=int(m.cur_ts), diff_travel_dist_local=float(m.diff_travel_dist_local),
                local_neural_points=c(m.local_neural_points), local_point_orientations=c(m.local_point_orientations),
                local_geo_features=c(m.local_geo_features), local_point_certainties=c(m.local_point_certainties),
                local_point_ts_update=c(m.local_point_ts_update), global2local=c(m.global2local),
                neighbor_dx=c(m.neighbor_dx), max_valid_dist2=m.max_valid_dist2, resolution=m.resolution,
                after_pgo=False, temporal_local_map_on=bool(m.temporal_local_map_on), nn_k=m.nn_k, weighted_first=False)


@pytest.mark.gpu
def test_hip_query_sees_points_inserted_by_hip_update(monkeypatch):
    """`pings_map_update` writes the hash table through its raw pointer, which torch's version
    counter cannot see; the query path's compact mirror must still follow.  update -> query -> update (new points,
    overwritten slots) -> query on ONE map object: compact-mirror results == dense-table results == CPU oracle."""
    from pings_amd import neural_map as NM
    from pings_amd import neural_points as hnp

    g = torch.Generator().manual_seed(9)
    m = NM.new_map(200_003, 8, 4, 0.25, temporal_local_map_on=True, local_map_radius=30.0,
                   sorrounding_map_radius=40.0, diff_travel_dist_local=100.0, device="cuda")   # small table: collisions
    m.geo_feature_std = 0.05
    m.travel_dist = torch.arange(4, dtype=torch.float32, device="cuda")
    _dress_map(m)
    dec = _Dec({"dec.layers.0.weight": 0.3 * torch.randn(64, 11, generator=g).numpy(),
                "dec.layers.0.bias": 0.1 * torch.randn(64, generator=g).numpy(),
                "dec.lout.weight": 0.3 * torch.randn(1, 64, generator=g).numpy(),
                "dec.lout.bias": np.zeros(1, np.float32), "sdf_scale": 0.03})
    sensor = torch.zeros(3, device="cuda")
    seen = []
    for ts in range(3):
        xy = (torch.rand(40_000, 2, generator=g) - 0.5) * 24.0 + torch.tensor([6.0 * ts, 0.0])
        pts = torch.cat([xy, (torch.sin(0.5 * xy[:, :1]) + 0.01 * torch.randn(40_000, 1, generator=g))], 1).cuda()
        NM.update(m, pts, torch.rand(40_000, 3, generator=g).cuda(), None, sensor, None, cur_ts=ts)
        n = int(m.neural_points.shape[0])
        seen.append(n)
        x = (m.neural_points[torch.randint(0, n, (3000,), generator=g).cuda()]
             + 0.1 * torch.randn(3000, 3, generator=g).cuda()).contiguous()
        monkeypatch.setattr(hnp, "USE_COMPACT_TABLE", True)
        hi, hd, hc = hnp.radius_neighborhood_topk(m, x, time_filtering=True, query_locally=True)
        s_c, _, c_c, _ = hnp.sdf_fused(m, dec, x)
        monkeypatch.setattr(hnp, "USE_COMPACT_TABLE", False)
        di, dd, dc = hnp.radius_neighborhood_topk(m, x, time_filtering=True, query_locally=True)
        s_d, _, c_d, _ = hnp.sdf_fused(m, dec, x)
        assert torch.equal(hi, di) and torch.equal(hd, dd) and torch.equal(hc, dc), f"frame {ts}: stale mirror"
        assert torch.equal(s_c, s_d) and torch.equal(c_c, c_d)
        cpu = sdf_cpu.NeuralPointMap(_state_of(m))
        ri, rd, rc = cpu.search_topk(x.cpu())
        assert torch.equal(hi.cpu(), ri) and torch.equal(hc.cpu(), rc) and torch.equal(hd.cpu(), rd)
        # the newest points are found: a query sitting exactly on the last inserted point returns it first
        last = m.neural_points[n - 1:n].contiguous()
        li, ld, _ = hnp.radius_neighborhood_topk(m, last, time_filtering=True, query_locally=False,
                                                 use_only_measured_points=False)
        assert int(li[0, 0]) == n - 1 and float(ld[0, 0]) == 0.0
    assert seen[0] < seen[1] < seen[2]


@pytest.mark.gpu
def test_hip_fused_sdf_5m_point_map_against_oracle():
    """BASELINE.json config C5 shape on one GPU (5M neural points, 1e8-slot table, K=81, k=6): neighbour indices,
    counts and fp32 squared distances index-/bit-exact on 4,096 queries vs oracle/sdf_cpu.py, SDF <= 1e-4."""
    from pings_amd import neural_points as hnp

    st, dec = sdf_cpu.synthetic_map(5_000_000)
    x = sdf_cpu.synthetic_queries(st, 4096)
    cpu = sdf_cpu.NeuralPointMap({**st})
    assert cpu.neural_points.shape[0] == 5_000_000
    ri, rd, rc = cpu.search_topk(x, use_only_measured_points=False)
    s_ref, _ = sdf_cpu.mapper_sdf(cpu, sdf_cpu.MLP.from_state({**dec}), x)
    del cpu
    gpu = _gpu_map({**st})
    hi, hd, hc = hnp.radius_neighborhood_topk(gpu, x.cuda(), query_locally=True)
    assert torch.equal(hi.cpu(), ri) and torch.equal(hc.cpu(), rc) and torch.equal(hd.cpu(), rd)
    sdf, grad, cnt, _ = hnp.sdf_fused(gpu, _Dec({**dec}), x.cuda(), need_grad=True, use_only_measured_points=False)
    assert rel_err(sdf, s_ref) <= 1e-4 and torch.isfinite(grad).all()
    assert float((cnt > 0).float().mean()) > 0.95


# ------------------------------------------------------------------ query_feature kernels: first and second order
def _qf_losses(npm, x, tabs, qf, seed=5):
    """A scalar of every differentiable output of query_feature, its gradient w.r.t. the query (create_graph) and a
    second scalar of that gradient: returns (first-order grads, second-order grads) w.r.t. (x, geo table, colour table)."""
    geo, col, w, cnt, cert = qf(npm, x, None, accumulate_stability=False, query_locally=True, query_color_feature=True)
    g = torch.Generator().manual_seed(seed)
    dev = x.device
    A = torch.randn(geo.shape, generator=g).to(dev)
    Bc = torch.randn(col.shape, generator=g).to(dev)
    Cw = torch.randn(w.shape, generator=g).to(dev)
    D = torch.randn(x.shape, generator=g).to(dev)
    L1 = (torch.tanh(geo) * A).sum() + (torch.sin(col) * Bc).sum() + (w ** 2 * Cw).sum()
    first = torch.autograd.grad(L1, [x] + tabs, create_graph=True, allow_unused=True)
    L2 = (first[0] * D).sum() + 0.3 * (first[0] ** 2).sum()
    second = torch.autograd.grad(L2, [x] + tabs, allow_unused=True)
    return (geo, col, w), first, second


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_query_feature_first_and_second_order_gradients_match_oracle(golden_dir, name):
    """`pings_query_feature_backward` / `_double_backward` (geo + colour tables, weights, neighbour vectors; both
    weighted_first modes, after_pgo rotations) against torch autograd through the oracle's op sequence — itself
    pinned to the reference by G2 / G3."""
    from pings_amd import neural_points as hnp

    st = load(golden_dir, name)
    cpu = sdf_cpu.NeuralPointMap(st)
    cpu.local_geo_features.requires_grad_(True)
    cpu.local_color_features.requires_grad_(True)
    xc = T(st["x"]).clone().requires_grad_(True)
    ref_out, ref1, ref2 = _qf_losses(cpu, xc, [cpu.local_geo_features, cpu.local_color_features],
                                     lambda m, x, ts, **kw: m.query_feature(x, ts, **kw))
    gpu = _gpu_map(st)
    gpu.local_geo_features.requires_grad_(True)
    gpu.local_color_features.requires_grad_(True)
    xg = T(st["x"]).cuda().requires_grad_(True)
    out, got1, got2 = _qf_losses(gpu, xg, [gpu.local_geo_features, gpu.local_color_features],
                                 lambda m, x, ts, **kw: hnp.query_feature(m, x, ts, **kw))
    for a, b, nm in zip(out, ref_out, ["geo", "colour", "w"]):
        assert rel_err(a, b) <= 1e-5, nm
    for a, b, nm in zip(got1, ref1, ["d x", "d geo table", "d colour table"]):
        assert rel_err(a, b) <= 1e-4, nm
    for a, b, nm in zip(got2, ref2, ["dd x", "dd geo table", "dd colour table"]):
        if b is None or float(b.abs().max()) == 0.0:    # per-neighbour mode: the backward does not read the tables
            assert a is None or float(a.abs().max()) == 0.0, nm
        else:
            assert rel_err(a, b) <= 2e-4, (nm, rel_err(a, b))   # second derivatives of 1/d^2 weights in fp32
    # reproducible: the scatter uses no float atomics
    _, again1, _ = _qf_losses(gpu, xg, [gpu.local_geo_features, gpu.local_color_features],
                              lambda m, x, ts, **kw: hnp.query_feature(m, x, ts, **kw))
    for a, b in zip(got1, again1):
        assert torch.equal(a, b)
    # a query without a gradient of its own (the mapper's sample points) takes the one-node path: same outputs, same
    # table gradients, bit for bit
    rw = torch.Generator().manual_seed(11)
    outs = []
    for needs_x in (True, False):
        xq = T(st["x"]).cuda().requires_grad_(needs_x)
        geo, col, w, cnt, cert = hnp.query_feature(gpu, xq, None, accumulate_stability=False, query_color_feature=True)
        if not outs:
            r_g = torch.randn(geo.shape, generator=rw).cuda()
            r_c = torch.randn(col.shape, generator=rw).cuda()
        loss = (geo * r_g).sum() + (col * r_c).sum()
        outs.append((geo.detach(), col.detach(), w.detach(), cnt, cert,
                     torch.autograd.grad(loss, [gpu.local_geo_features, gpu.local_color_features])))
    for a, b in zip(outs[0][:5], outs[1][:5]):
        assert torch.equal(a, b)
    for a, b in zip(outs[0][5], outs[1][5]):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_rows_scatter_add_is_exact_and_reproducible():
    """`pings_rows_scatter_add` vs a float64 index_add: hot rows (one row receiving 3,000 pairs), skipped pairs,
    weights, source-row indirection, every F the feature tables use."""
    from pings_amd import neural_points as hnp

    g = torch.Generator().manual_seed(2)
    rows, n = 5000, 40_000
    for F, ld in ((8, 11), (16, 19), (32, 35), (4, 4), (61, 64)):
        dst = torch.randint(0, rows, (n,), generator=g)
        dst[:3000] = 17                                  # a hot row
        dst[torch.randint(0, n, (500,), generator=g)] = -1   # skipped
        src = torch.randn(n, ld, generator=g)
        w = torch.rand(n, generator=g)
        ref = torch.zeros(rows, F, dtype=torch.float64)
        ok = dst >= 0
        ref.index_add_(0, dst[ok], (src[ok, :F].double() * w[ok, None].double()))
        a = hnp.rows_scatter_add(dst.cuda(), src.cuda(), rows, w=w.cuda(), F=F)
        b = hnp.rows_scatter_add(dst.cuda(), src.cuda(), rows, w=w.cuda(), F=F)
        assert torch.equal(a, b)
        assert rel_err(a, ref) <= 1e-5, F
        # source-row indirection without weights: pair p reads row p // 4
        sr = torch.arange(n) // 4
        ref2 = torch.zeros(rows, F, dtype=torch.float64)
        ref2.index_add_(0, dst[ok], src[sr[ok], :F].double())
        c = hnp.rows_scatter_add(dst.cuda(), src.cuda(), rows, src_row=sr.cuda(), F=F)
        assert rel_err(c, ref2) <= 1e-5, F
    # no pairs at all: a table of zeros
    z = hnp.rows_scatter_add(torch.empty(0, dtype=torch.int64, device="cuda"), torch.empty(0, 8, device="cuda"), 10)
    assert z.shape == (10, 8) and float(z.abs().max()) == 0.0


# ------------------------------------------------------------------ fused Mapper.sdf: first and second order
class _FakeMapper:
    """The attributes `pings_amd.mapper_ops` reads from the reference's Mapper."""

    def __init__(self, npm, dec):
        from types import SimpleNamespace as NS

        self.neural_points, self.sdf_mlp = npm, dec
        self.config = NS(weighted_first=npm.weighted_first)
        self.dtype, self.device = torch.float32, "cuda"


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_fused_mapper_sdf_double_backward_matches_reference_golden(golden_dir, name):
    """`Mapper.sdf` + `get_gradient(create_graph=True)` + backward (utils/mapper.py:1445-1448, the G3 vectors) through
    the FUSED kernels: pings_sdf_forward -> pings_sdf_backward / pings_sdf_double_backward, no torch op in between."""
    from types import SimpleNamespace as NS

    from pings_amd import mapper_ops

    st = load(golden_dir, name)
    gpu = _gpu_map(st)
    gpu.local_geo_features.requires_grad_(True)
    t = lambda k: torch.nn.Parameter(T(st["dec." + k]).cuda())
    d = NS(layers=[NS(weight=t("layers.0.weight"), bias=t("layers.0.bias"))],
           lout=NS(weight=t("lout.weight"), bias=t("lout.bias")), sdf_scale=float(st["sdf_scale"]), use_leaky_relu=False)
    m = _FakeMapper(gpu, d)
    params = [gpu.local_geo_features, d.layers[0].weight, d.layers[0].bias, d.lout.weight, d.lout.bias]
    outs = []
    for _ in range(2):
        x = T(st["x"]).cuda().requires_grad_(True)
        s, _, valid = mapper_ops.sdf(m, x, min_nn_count=1)
        g = sdf_cpu.get_gradient(x, s)
        loss = ((g.norm(dim=-1) - 1.0) ** 2).mean() + s.abs().mean()
        outs.append(torch.autograd.grad(loss, params))
    assert rel_err(s, T(st["g3_sdf"])) <= 1e-4
    assert rel_err(g, T(st["g3_grad_x"])) <= 1e-4
    assert abs(loss.item() - float(st["g3_loss"])) <= 1e-4 * max(1.0, abs(float(st["g3_loss"])))
    names = ["g3_dfeat", "g3_d.layers.0.weight", "g3_d.layers.0.bias", "g3_d.lout.weight", "g3_d.lout.bias"]
    for a, k in zip(outs[0], names):
        assert rel_err(a.reshape(T(st[k]).shape), T(st[k])) <= 1e-4, (k, rel_err(a.reshape(T(st[k]).shape), T(st[k])))
    for a, b in zip(*outs):
        assert torch.equal(a, b)                                   # bitwise reproducible
    # inference forms agree with the training form
    with torch.no_grad():
        s2, std, v2 = mapper_ops.sdf(m, T(st["x"]).cuda(), get_std=True)
        s3, _, v3 = mapper_ops.sdf_batch(m, T(st["x"]).cuda(), 1000)
    assert torch.equal(s2, s.detach()) and torch.equal(s3, s2) and torch.equal(v2, valid) and torch.equal(v3, valid)
    # numerical gradient: six shifted queries in one launch, differentiable to the parameters
    xq = T(st["x"]).cuda()[:512]
    gn = mapper_ops.get_numerical_gradient(m, xq, eps=0.05)
    cpu = sdf_cpu.NeuralPointMap(st)
    dec_c = sdf_cpu.MLP.from_state(st)
    e = torch.eye(3) * 0.05
    xc = T(st["x"])[:512]
    ref = torch.cat([(sdf_cpu.mapper_sdf(cpu, dec_c, xc + e[i])[0] - sdf_cpu.mapper_sdf(cpu, dec_c, xc - e[i])[0])[:, None] / 0.1
                     for i in range(3)], 1)
    assert rel_err(gn, ref) <= 1e-3          # difference quotient of fp32 values: cancellation
    torch.autograd.grad(gn.square().sum(), params)


@pytest.mark.gpu
@pytest.mark.parametrize("two_side", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_fused_numerical_gradient_equals_the_reference_op_sequence(golden_dir, name, two_side):
    """`get_numerical_gradient` as one graph node (stencil kernels around the fused query) against the reference's own
    tensor-op sequence (utils/mapper.py:2319-2370) evaluated on the device: values and all parameter gradients."""
    from types import SimpleNamespace as NS

    from pings_amd import mapper_ops

    st = load(golden_dir, name)
    gpu = _gpu_map(st)
    gpu.local_geo_features.requires_grad_(True)
    t = lambda k: torch.nn.Parameter(T(st["dec." + k]).cuda())
    d = NS(layers=[NS(weight=t("layers.0.weight"), bias=t("layers.0.bias"))],
           lout=NS(weight=t("lout.weight"), bias=t("lout.bias")), sdf_scale=float(st["sdf_scale"]), use_leaky_relu=False)
    m = _FakeMapper(gpu, d)
    params = [gpu.local_geo_features, d.layers[0].weight, d.layers[0].bias, d.lout.weight, d.lout.bias]
    xq = T(st["x"]).cuda()[:700]
    eps = 0.05
    up = torch.randn(700, 3, generator=torch.Generator().manual_seed(4)).cuda()

    def run(x):
        s0 = mapper_ops.sdf(m, x.detach())[0] if not two_side else None
        g = mapper_ops.get_numerical_gradient(m, x, s0, eps=eps, two_side=two_side)
        return g, torch.autograd.grad((g * up).sum(), params + ([s0] if s0 is not None and s0.requires_grad else []),
                                      allow_unused=True)

    g_f, d_f = run(xq)                                      # fused node
    assert type(g_f.grad_fn).__name__ == "_NumGradBackward"
    g_c, d_c = run(xq.clone().requires_grad_(True))         # composed path: the reference's op sequence on the fused sdf
    assert type(g_c.grad_fn).__name__ != "_NumGradBackward"
    # the composed path differentiates x as well, i.e. runs the forward kernel variant that also produces dS/dx: its S
    # agrees to fp32 rounding, which the difference quotient (/ eps) amplifies
    assert rel_err(g_f, g_c) <= 1e-4, rel_err(g_f, g_c)
    for a, b in zip(d_f, d_c):
        # (the output bias cancels in a difference quotient: its gradient is an fp32 sum of +v and -v terms, ~1e-5)
        assert (a - b).abs().max().item() <= 1e-4 * max(b.abs().max().item(), 1.0), (a - b).abs().max().item()
    with torch.no_grad():
        g_n = mapper_ops.get_numerical_gradient(m, xq, mapper_ops.sdf(m, xq)[0], eps=eps, two_side=two_side)
    assert torch.equal(g_n, g_f.detach())
    # an empty batch (every Eikonal sample masked out) returns an empty gradient, as the reference's ops do
    e = mapper_ops.get_numerical_gradient(m, xq[:0], mapper_ops.sdf(m, xq)[0][:0], eps=eps, two_side=two_side)
    assert e.shape == (0, 3)


@pytest.mark.gpu
def test_query_feature_on_an_empty_batch_returns_empty_tensors(golden_dir):
    """model/neural_gaussians.py:506-725 on zero query points returns empty tensors."""
    from pings_amd import neural_points as hnp

    st = load(golden_dir, CASES[0])
    gpu = _gpu_map(st)
    x = T(st["x"]).cuda()[:0]
    geo, col, w, cnt, cert = hnp.query_feature(gpu, x, accumulate_stability=True)
    assert geo.shape[0] == 0 and w.shape[0] == 0 and cnt.shape[0] == 0


# ------------------------------------------------------------------ options no shipped config sets (VERDICT r2 missing #5)
@pytest.mark.gpu
@pytest.mark.parametrize("weighted_first", [False, True])
def test_layer_norm_on_runs_through_the_kernels_and_torch_layer_norm(golden_dir, weighted_first):
    """config.layer_norm_on (utils/config.py:95; model/neural_gaussians.py:591-592): `F.layer_norm` over the gathered
    feature rows before the neighbour vector is appended and before the weighted sum.  The HIP kernels deliver the rows,
    the normalisation is torch's on the device; checked against the same composition written out, with gradients."""
    from pings_amd import neural_points as hnp

    st = load(golden_dir, "gs_f32")
    gpu = _gpu_map(st)
    gpu.local_geo_features.requires_grad_(True)
    x = T(st["x"]).cuda()[:900]
    F_ = gpu.local_geo_features.shape[1]
    gpu.config.weighted_first, gpu.config.layer_norm_on = False, False
    rows, _, w, cnt, _ = hnp.query_feature(gpu, x, accumulate_stability=False)
    exp = torch.cat((torch.nn.functional.layer_norm(rows[..., :F_], [F_]), rows[..., F_:]), -1)
    if weighted_first:
        exp = (exp * w).sum(1)
    g_exp = torch.autograd.grad(exp.square().sum(), gpu.local_geo_features)[0]
    gpu.config.weighted_first, gpu.config.layer_norm_on = weighted_first, True
    got, _, w2, cnt2, _ = hnp.query_feature(gpu, x, accumulate_stability=False)
    g_got = torch.autograd.grad(got.square().sum(), gpu.local_geo_features)[0]
    assert got.shape == exp.shape and torch.equal(cnt, cnt2) and torch.equal(w, w2)
    assert rel_err(got, exp) <= 1e-6 and rel_err(g_got, g_exp) <= 1e-5
    # rows of queries without neighbours stay exactly zero through the layer norm (:585-592 normalises zero rows to zero)
    assert float(got[cnt == 0].abs().sum()) == 0.0


class _DeepLeakyDecoder(torch.nn.Module):
    """model/decoder.py with `mlp_level` 2 and `mlp_leaky_relu` (utils/config.py:145-146): outside the fused kernels."""

    def __init__(self, IN, HID, scale):
        super().__init__()
        torch.manual_seed(5)
        self.layers = torch.nn.ModuleList([torch.nn.Linear(IN, HID), torch.nn.Linear(HID, HID)])
        self.lout = torch.nn.Linear(HID, 1)
        self.use_leaky_relu, self.sdf_scale = True, scale

    def mlp(self, f):
        h = f
        for l in self.layers:
            h = torch.nn.functional.leaky_relu(l(h))
        return self.lout(h)

    def sdf(self, f):
        return self.mlp(f).squeeze(1) * self.sdf_scale


@pytest.mark.gpu
def test_decoders_outside_the_fused_kernels_take_the_composed_path(golden_dir):
    """Two hidden levels + leaky ReLU: `Mapper.sdf`, `sdf_fused` (tracker / mesher) and `get_numerical_gradient` return what
    `query_feature` -> `Decoder.sdf` -> IDW sum gives (utils/mapper.py:2273-2289), with gradients, instead of raising."""
    from types import SimpleNamespace as NS

    from pings_amd import mapper_ops, neural_points as hnp

    st = load(golden_dir, "gs_f32")
    gpu = _gpu_map(st)
    gpu.local_geo_features.requires_grad_(True)
    dec = _DeepLeakyDecoder(gpu.local_geo_features.shape[1] + 3, 48, float(st["sdf_scale"])).cuda()
    assert not hnp.fused_supported(gpu, dec)
    m = _FakeMapper(gpu, dec)
    x = T(st["x"]).cuda()[:800]
    geo, _, w, cnt, _ = hnp.query_feature(gpu, x, accumulate_stability=False)
    ref = (dec.sdf(geo) * w).sum(1).squeeze(1)
    g_ref = torch.autograd.grad(ref.abs().sum(), [gpu.local_geo_features, *dec.parameters()])
    s, std, valid = mapper_ops.sdf(m, x, get_std=False)
    g = torch.autograd.grad(s.abs().sum(), [gpu.local_geo_features, *dec.parameters()])
    assert rel_err(s, ref) <= 1e-6 and torch.equal(valid, cnt >= 1)
    for a, b in zip(g, g_ref):
        assert rel_err(a, b) <= 1e-5
    xg = x.clone().requires_grad_(True)
    geo2, _, w2, _, _ = hnp.query_feature(gpu, xg, accumulate_stability=False)
    gx_ref = torch.autograd.grad((dec.sdf(geo2) * w2).sum(1).sum(), xg)[0]
    s2, gx, cnt2, cert, sd = hnp.sdf_fused(gpu, dec, x, need_grad=True, need_certainty=True, need_std=True)
    assert rel_err(s2, ref) <= 1e-6 and rel_err(gx, gx_ref) <= 1e-5 and torch.equal(cnt2, cnt) and sd.shape == s2.shape
    gn = mapper_ops.get_numerical_gradient(m, x[:200], eps=0.05)
    assert gn.shape == (200, 3) and torch.isfinite(gn).all()


# ------------------------------------------------------------------ cell-block index (csrc/knn_blocks.hip)
def _search_all_modes(cpu, gpu, x, hnp):
    out = []
    for local, meas, val in [(True, True, False), (False, True, True), (False, False, False), (True, False, True)]:
        ref = cpu.search_topk(x, query_locally=local, use_only_measured_points=meas, use_only_valid_points=val)
        got = hnp.radius_neighborhood_topk(gpu, x.cuda(), time_filtering=cpu.temporal_local_map_on and local,
                                           use_only_measured_points=meas, use_only_valid_points=val,
                                           query_locally=local)
        out.append((ref, got))
    return out


def _assert_search_equal(pairs):
    for (ri, rd, rc), (hi, hd, hc) in pairs:
        assert torch.equal(hc.cpu(), rc) and torch.equal(hi.cpu(), ri) and torch.equal(hd.cpu(), rd)


@pytest.mark.gpu
@pytest.mark.parametrize("index", ["blocks", "table"])
@pytest.mark.parametrize("name", CASES)
def test_hip_search_layouts_give_the_reference_neighbours(golden_dir, name, index, monkeypatch):
    """Both search-side layouts (cell-block index, the reference's table) against the oracle on the reference's
    own maps: indices, order, distances and counts bit for bit, in all four mask / local modes."""
    from pings_amd import neural_points as hnp

    monkeypatch.setattr(hnp, "KNN_INDEX", index)
    st = load(golden_dir, name)
    cpu, gpu = sdf_cpu.NeuralPointMap(st), _gpu_map(st)
    _assert_search_equal(_search_all_modes(cpu, gpu, T(st["x"]), hnp))
    if index == "blocks":
        status = hnp._block_index(gpu).status.cpu().tolist()
        assert status[0] == 1 and status[1] == status[2] == status[4] and status[3] == 0


@pytest.mark.gpu
def test_block_index_masks_random_and_stale(monkeypatch):
    """Random free / valid masks, a partial local map and a time window on a synthetic map; then in-place changes of
    the baked tensors must be seen by the next query (the index is keyed on torch's version counters)."""
    from pings_amd import neural_points as hnp

    monkeypatch.setattr(hnp, "KNN_INDEX", "blocks")
    st, _ = sdf_cpu.synthetic_map(20000, seed=3)
    n = st["neural_points"].shape[0]
    rng = np.random.default_rng(0)
    st["free_gs_mask"] = rng.random(n) < 0.2
    st["valid_gs_mask"] = rng.random(n) < 0.8
    g2l = np.full(n + 1, -1, np.int64)
    keep = np.flatnonzero(rng.random(n) < 0.7)
    g2l[keep] = np.arange(keep.shape[0])
    st["global2local"] = g2l
    st["point_ts_create"] = rng.integers(0, 50, n).astype(np.int32)
    st["travel_dist"] = np.cumsum(rng.random(50)).astype(np.float32)
    st["cur_ts"], st["diff_travel_dist_local"], st["temporal_local_map_on"] = 49, 12.0, True
    cpu, gpu = sdf_cpu.NeuralPointMap({**st}), _gpu_map({**st})
    assert cpu.temporal_local_map_on
    x = sdf_cpu.synthetic_queries(st, 3000)
    x = torch.cat([x, torch.tensor([[1e7, 0, 0], [-3e6, 2e6, 5.0], [0, 0, 1e4]])])   # far outside any cell
    _assert_search_equal(_search_all_modes(cpu, gpu, x, hnp))
    assert hnp._block_index(gpu).status.cpu().tolist()[0] == 1
    first = hnp._block_index(gpu)
    # in-place edits of baked tensors, mirrored on the oracle's copy
    flip = torch.from_numpy(rng.random(n) < 0.3)
    cpu.valid_gs_mask[flip] = ~cpu.valid_gs_mask[flip]
    gpu.valid_gs_mask[flip.cuda()] = ~gpu.valid_gs_mask[flip.cuda()]
    cpu.free_gs_mask[:100] = True
    gpu.free_gs_mask[:100] = True
    cpu.global2local[keep[:500]] = -1
    gpu.global2local[torch.from_numpy(keep[:500]).cuda()] = -1
    _assert_search_equal(_search_all_modes(cpu, gpu, x, hnp))
    second = hnp._block_index(gpu)
    assert second is not first
    # a per-frame tensor REPLACED by a new object of the same shape / dtype / version counter (what reset_local_map
    # does to global2local every frame; the allocator may even hand out the old address): identity decides
    g2 = torch.full_like(cpu.global2local, -1)
    g2[torch.from_numpy(keep[600:])] = torch.arange(keep.shape[0] - 600)
    cpu.global2local = g2
    gpu.global2local = g2.cuda()
    _assert_search_equal(_search_all_modes(cpu, gpu, x, hnp))
    assert hnp._block_index(gpu) is not second


@pytest.mark.gpu
def test_block_index_refuses_tables_it_cannot_mirror(monkeypatch):
    """(b) a 76,273-slot table: cells (2, 1, -2) apart share a slot (2 P0 + P1 - 2 P2 = 76,273), the host check fails
    (a 20,011-slot table, by contrast, only collides far-away cells and IS mirrored); (a) a slot holding a point of another
    cell: registered points != non-empty slots.  status[0] stays 0 and the kernels answer from the table — still the
    oracle's neighbours."""
    from pings_amd import neural_points as hnp

    monkeypatch.setattr(hnp, "KNN_INDEX", "blocks")
    for size, ok in ((76273, 0), (20011, 1)):
        st, _ = sdf_cpu.synthetic_map(3000, buffer_size=size)
        cpu, gpu = sdf_cpu.NeuralPointMap({**st}), _gpu_map({**st})
        x = sdf_cpu.synthetic_queries(st, 1000)
        _assert_search_equal(_search_all_modes(cpu, gpu, x, hnp))
        assert hnp._block_index(gpu).status.cpu().tolist()[0] == ok

    st, _ = sdf_cpu.synthetic_map(5000, seed=9)
    cpu, gpu = sdf_cpu.NeuralPointMap({**st}), _gpu_map({**st})
    # the slot of point 10's cell now holds its neighbour in the list, point 11 (close enough to pass the distance test)
    slot10 = int((cpu.buffer_pt_index == 10).nonzero()[0, 0])
    cpu.buffer_pt_index[slot10] = 11
    gpu.buffer_pt_index[slot10] = 11
    x = torch.cat([sdf_cpu.synthetic_queries(st, 1000), cpu.neural_points[8:14] + 0.01])
    _assert_search_equal(_search_all_modes(cpu, gpu, x, hnp))
    status = hnp._block_index(gpu).status.cpu().tolist()
    assert status[0] == 0 and status[1] == status[2] - 1


@pytest.mark.gpu
@pytest.mark.parametrize("F,H,nn_k", [(8, 32, 6), (16, 64, 8), (4, 16, 3), (32, 48, 6)])
def test_matrix_core_sdf_kernels_other_decoder_shapes(F, H, nn_k, monkeypatch):
    """The matrix-core forward / backward of the fused SDF query on decoder shapes the golden maps do not have (one
    hidden block, 12- and 20-wide padded inputs, a ragged hidden width, nn_k = 8 and 3): against the vector kernels
    (which the golden tests pin) and against the oracle."""
    from types import SimpleNamespace as NS

    from pings_amd import neural_points as hnp

    st, dec = sdf_cpu.synthetic_map(6000, feat_dim=F, hidden=H, nn_k=nn_k, seed=F + H)
    x = sdf_cpu.synthetic_queries(st, 1501)          # not a multiple of four: the last wave step is ragged
    cpu, gpu = sdf_cpu.NeuralPointMap({**st}), _gpu_map({**st})
    s_ref, _ = sdf_cpu.mapper_sdf(cpu, sdf_cpu.MLP.from_state({**dec}), x)
    gw = torch.randn(x.shape[0], generator=torch.Generator().manual_seed(1)).cuda()
    res = {}
    for mode in ("mfma", "vector"):
        monkeypatch.setenv("PINGS_SDF_FWD", mode)
        monkeypatch.setenv("PINGS_SDF_BWD", mode)
        # the default plan of these shapes is the matrix-core family: the two runs are two different kernels
        assert gpu.local_geo_features.data_ptr() % 16 == 0
        for order in (FWD, BWD):
            assert _plan(nn_k, F, H, False, order)[0] == (MATRIX if mode == "mfma" else VECTOR)
        out = hnp.sdf_fused(gpu, _Dec({**dec}), x.cuda(), need_grad=True, need_std=True,
                            use_only_measured_points=False)
        feats = gpu.local_geo_features.detach().clone().requires_grad_(True)
        gpu.local_geo_features = feats
        P = [torch.nn.Parameter(torch.as_tensor(dec["dec." + k]).cuda().clone()) for k in
             ("layers.0.weight", "layers.0.bias", "lout.weight", "lout.bias")]
        d = NS(layers=[NS(weight=P[0], bias=P[1])], lout=NS(weight=P[2], bias=P[3]),
               sdf_scale=float(_Dec({**dec}).sdf_scale), use_leaky_relu=False)
        s, _ = hnp.sdf_train(gpu, d, x.cuda(), use_only_measured_points=False)
        grads = torch.autograd.grad((s * gw).sum(), [feats] + P)
        res[mode] = (out, s.detach(), grads)
    assert rel_err(res["mfma"][1], s_ref) <= 1e-4 and rel_err(res["vector"][1], s_ref) <= 1e-4
    for a, b in zip(res["mfma"][0], res["vector"][0]):
        if a is None:
            continue
        assert torch.equal(a, b) if a.dtype == torch.int64 else rel_err(a, b) <= 2e-5
    for a, b in zip(res["mfma"][2], res["vector"][2]):
        assert rel_err(a, b) <= 5e-5, rel_err(a, b)
    # tiny batches: every fill level of the last four-query wave step
    ref_s = res["vector"][1]
    monkeypatch.setenv("PINGS_SDF_FWD", "mfma")
    monkeypatch.setenv("PINGS_SDF_BWD", "mfma")
    for nb in (1, 2, 3, 5):
        s_small, _, cnt_small, _ = hnp.sdf_fused(gpu, _Dec({**dec}), x[:nb].cuda(), use_only_measured_points=False)
        assert torch.equal(s_small, res["mfma"][0][0][:nb]) and rel_err(s_small, ref_s[:nb]) <= 2e-5
        assert torch.equal(cnt_small, res["mfma"][0][2][:nb])


# ------------------------------------------------------------------ the launch plan of the fused query (csrc/sdf_plan.hpp)
def _expected_plan(nn_k, F, H, weighted_first, order, misaligned):
    """The plan as DESIGN states it: matrix core for the per-neighbour decoder with nn_k <= 8 and 4, 8, 16 or 32 aligned
    features, forward and first-order backward only; classes by padded input width."""
    if order != BWD2 and not weighted_first and not misaligned and nn_k <= 8 and H <= 64 and F in (4, 8, 16, 32):
        need = F + 4
        return MATRIX, 12 if need <= 12 else 20 if need <= 20 else 36
    n = F + 3
    if order == FWD:
        return VECTOR, 12 if n <= 12 else 36 if n <= 36 else 64
    return VECTOR, 12 if n <= 12 else 20 if n <= 20 else 36 if n <= 36 else 64


@pytest.mark.parametrize("F,fwd,bwd,bwd2", [
    (9, (VECTOR, 12), (VECTOR, 12), (VECTOR, 12)), (10, (VECTOR, 36), (VECTOR, 20), (VECTOR, 20)),
    (17, (VECTOR, 36), (VECTOR, 20), (VECTOR, 20)), (18, (VECTOR, 36), (VECTOR, 36), (VECTOR, 36)),
    (33, (VECTOR, 36), (VECTOR, 36), (VECTOR, 36)), (34, (VECTOR, 64), (VECTOR, 64), (VECTOR, 64)),
    (61, (VECTOR, 64), (VECTOR, 64), (VECTOR, 64)),
    (4, (MATRIX, 12), (MATRIX, 12), (VECTOR, 12)), (8, (MATRIX, 12), (MATRIX, 12), (VECTOR, 12)),
    (16, (MATRIX, 20), (MATRIX, 20), (VECTOR, 20)), (32, (MATRIX, 36), (MATRIX, 36), (VECTOR, 36)),
    (12, (VECTOR, 36), (VECTOR, 20), (VECTOR, 20)),          # F / 4 = 3 is not a power of two
])
def test_sdf_plan_at_both_sides_of_every_threshold(F, fwd, bwd, bwd2, monkeypatch):
    monkeypatch.delenv("PINGS_SDF_FWD", raising=False)
    monkeypatch.delenv("PINGS_SDF_BWD", raising=False)
    assert [_plan(6, F, 64, False, o) for o in (FWD, BWD, BWD2)] == [fwd, bwd, bwd2]
    vec = [(VECTOR, c) for c in (_expected_plan(6, F, 64, True, o, False)[1] for o in (FWD, BWD, BWD2))]
    assert vec[2] == bwd2                                      # the second order is always the vector kernel
    assert [_plan(8, F, 64, False, o) for o in (FWD, BWD, BWD2)] == [fwd, bwd, bwd2]     # nn_k 8 | 9
    assert [_plan(9, F, 64, False, o) for o in (FWD, BWD, BWD2)] == vec
    assert [_plan(6, F, 64, True, o) for o in (FWD, BWD, BWD2)] == vec                   # weighted_first
    assert [_plan(6, F, 64, False, o, misaligned=True) for o in (FWD, BWD, BWD2)] == vec
    assert [_plan(6, F, 1, False, o) for o in (FWD, BWD, BWD2)] == [fwd, bwd, bwd2]      # hidden 1 .. 64 alike
    monkeypatch.setenv("PINGS_SDF_FWD", "vector")
    assert [_plan(6, F, 64, False, o) for o in (FWD, BWD, BWD2)] == [vec[0], bwd, bwd2]
    monkeypatch.setenv("PINGS_SDF_BWD", "vector")
    assert [_plan(6, F, 64, False, o) for o in (FWD, BWD, BWD2)] == vec
    monkeypatch.setenv("PINGS_SDF_FWD", "mfma")
    assert [_plan(6, F, 64, False, o) for o in (FWD, BWD, BWD2)] == [fwd, vec[1], vec[2]]


def test_sdf_plan_refuses_shapes_the_kernels_do_not_take():
    from pings_amd import _lib

    L, out = _lib.lib(), (ctypes.c_int32 * 2)()
    assert _plan(6, 32, 64) == (MATRIX, 36)                    # feat_dim 32 forward: class 36, never 64
    for nn_k, F, H, order in [(0, 32, 64, 0), (17, 32, 64, 0), (6, 0, 64, 0), (6, 62, 64, 0), (6, 32, 0, 0),
                              (6, 32, 65, 0), (6, 32, 64, 3), (6, 32, 64, -1)]:
        assert L.pings_sdf_plan(nn_k, F, H, 0, order, 0, out) == 1, (nn_k, F, H, order)
    assert L.pings_sdf_plan(6, 32, 64, 0, 0, 0, None) == 1


def _reachable_sdf_classes():
    """{(order, family): classes} of `pings_sdf_plan` swept over every admitted shape, each plan also checked against
    `_expected_plan`."""
    got = {}
    for F, nn_k, wf, mis, order, H in itertools.product(range(1, 62), range(1, 17), (False, True), (False, True),
                                                        (FWD, BWD, BWD2), (1, 37, 64)):
        fam, cls = _plan(nn_k, F, H, wf, order, mis)
        assert (fam, cls) == _expected_plan(nn_k, F, H, wf, order, mis), (nn_k, F, H, wf, order, mis)
        got.setdefault((order, fam), set()).add(cls)
    return got


def test_sdf_classes_built_are_the_classes_the_plan_can_return(monkeypatch):
    """The `with_class<...>` lists of the four SDF launches against the plan swept over every admitted shape: a class
    nobody can ask for fails, and so does a class asked for and not built."""
    monkeypatch.delenv("PINGS_SDF_FWD", raising=False)
    monkeypatch.delenv("PINGS_SDF_BWD", raising=False)
    built = mlp_ref.with_class_lists("knn_sdf.hip", "sdf_fwd_mfma.hip", "sdf_bwd.hip")
    assert sorted(built) == ["SDF backward", "SDF backward, matrix core", "SDF forward", "SDF forward, matrix core"]
    want = _reachable_sdf_classes()
    assert (BWD2, MATRIX) not in want                          # the second order has no matrix-core kernel
    assert want[(BWD, VECTOR)] == want[(BWD2, VECTOR)]         # one list, two instantiations (SECOND)
    assert built == {"SDF forward": want[(FWD, VECTOR)], "SDF forward, matrix core": want[(FWD, MATRIX)],
                     "SDF backward": want[(BWD, VECTOR)], "SDF backward, matrix core": want[(BWD, MATRIX)]}
    # and the GPU test below runs every one of them
    ran = {}
    for fam, F, H, nn_k, wf in PLAN_CASES:
        for order in (FWD, BWD, BWD2):
            for forced in ((False, True) if fam == MATRIX else (False,)):
                f, c = _expected_plan(nn_k, F, H, wf or forced, order, False)
                ran.setdefault((order, f), set()).add(c)
    assert ran == want


PLAN_CASES = [(VECTOR, 9, 64, 6, False), (VECTOR, 10, 33, 9, False), (VECTOR, 17, 64, 6, False),
              (VECTOR, 18, 64, 6, False), (VECTOR, 33, 64, 6, False), (VECTOR, 34, 17, 16, False),
              (VECTOR, 61, 64, 6, False), (VECTOR, 32, 64, 6, True),
              (MATRIX, 4, 16, 3, False), (MATRIX, 8, 32, 6, False), (MATRIX, 16, 64, 8, False),
              (MATRIX, 32, 48, 6, False)]


def _plan_case(F, H, nn_k, weighted_first):
    """Map, decoder, queries and the oracle's answers for one shape: forward (sdf, dS/dx, spread, counts), first-order
    gradients of sum(s * gw) and second-order gradients of the Eikonal loss w.r.t. (features, W1, b1, W2, b2).

    6,000 points.  The stock queries sit on the sheet and nearly all have MORE than nn_k candidates, so every third one
    is lifted off the sheet by 0.3 .. 1.3 (the search radius): their candidate counts run from many down to none, which
    gives every case queries with exactly nn_k candidates, with fewer, and with none."""
    st, dec = sdf_cpu.synthetic_map(6000, feat_dim=F, hidden=H, nn_k=nn_k, weighted_first=weighted_first, seed=F + H)
    x = sdf_cpu.synthetic_queries(st, 1501)          # not a multiple of four: the last wave step is ragged
    x[::3, 2] += torch.linspace(0.3, 1.3, x[::3].shape[0])
    cpu, d = sdf_cpu.NeuralPointMap({**st}), sdf_cpu.MLP.from_state({**dec})
    P = [cpu.local_geo_features] + d.parameters()
    for p in P:
        p.requires_grad_(True)
    xg = x.clone().requires_grad_(True)
    geo, _, w, cnt, _ = cpu.query_feature(xg, accumulate_stability=False)
    s = d.sdf(geo)
    std = torch.zeros_like(x[:, 0])
    if not weighted_first:
        std = torch.sqrt(torch.sum(w * (s - torch.sum(s * w, dim=1, keepdim=True)) ** 2, dim=1)).squeeze(1).detach()
        s = torch.sum(s * w, dim=1).squeeze(1)
    gw = torch.randn(x.shape[0], generator=torch.Generator().manual_seed(1))
    first = torch.autograd.grad((s * gw).sum(), P, retain_graph=True)
    g = sdf_cpu.get_gradient(xg, s)
    second = torch.autograd.grad(((g.norm(dim=-1) - 1.0) ** 2).mean() + s.abs().mean(), P)
    return st, dec, x, gw, dict(sdf=s.detach(), grad=g.detach(), std=std, cnt=cnt, first=first, second=second)


@pytest.mark.gpu
@pytest.mark.parametrize("family,F,H,nn_k,weighted_first", PLAN_CASES,
                         ids=[f"{'matrix' if c[0] else 'vector'}-F{c[1]}-H{c[2]}-k{c[3]}{'-wf' if c[4] else ''}"
                              for c in PLAN_CASES])
def test_every_sdf_kernel_class_against_the_oracle(family, F, H, nn_k, weighted_first, monkeypatch):
    """Every (family, class, order) `pings_sdf_plan` can return, on the shape at the edge of its class: forward with
    dS/dx and the spread, first-order training gradients, and the Eikonal loss's second-order pass, each against the
    oracle (1e-4) and, where the shape has a matrix-core kernel, against the vector kernel (2e-5 forward, 5e-5
    gradients; integer outputs equal).  Each run first asserts the kernel it claims to run."""
    from types import SimpleNamespace as NS

    from pings_amd import mapper_ops
    from pings_amd import neural_points as hnp

    st, dec, x, gw, ref = _plan_case(F, H, nn_k, weighted_first)
    assert (ref["cnt"] == nn_k).any() and ((ref["cnt"] > 0) & (ref["cnt"] < nn_k)).any()
    gpu = _gpu_map({**st})
    xc, gwc = x.cuda(), gw.cuda()
    names = ["features", "W1", "b1", "W2", "b2"]
    res, errs = {}, {}
    for mode in (("mfma", "vector") if family == MATRIX else ("mfma",)):
        monkeypatch.setenv("PINGS_SDF_FWD", mode)
        monkeypatch.setenv("PINGS_SDF_BWD", mode)
        fam = family if mode == "mfma" else VECTOR
        assert gpu.local_geo_features.data_ptr() % 16 == 0
        for order in (FWD, BWD, BWD2):
            assert _plan(nn_k, F, H, weighted_first, order) == \
                _expected_plan(nn_k, F, H, weighted_first or fam == VECTOR, order, False)
            assert _plan(nn_k, F, H, weighted_first, order)[0] == (fam if order != BWD2 else VECTOR)
        out = hnp.sdf_fused(gpu, _Dec({**dec}), xc, need_grad=True, need_std=True)
        feats = gpu.local_geo_features.detach().clone().requires_grad_(True)
        gpu.local_geo_features = feats
        P = [torch.nn.Parameter(torch.as_tensor(dec["dec." + k]).cuda().clone()) for k in
             ("layers.0.weight", "layers.0.bias", "lout.weight", "lout.bias")]
        d = NS(layers=[NS(weight=P[0], bias=P[1])], lout=NS(weight=P[2], bias=P[3]), sdf_scale=float(dec["sdf_scale"]),
               use_leaky_relu=False)
        s, _ = hnp.sdf_train(gpu, d, xc)
        first = torch.autograd.grad((s * gwc).sum(), [feats] + P)
        xg = xc.clone().requires_grad_(True)
        s2, _, _ = mapper_ops.sdf(_FakeMapper(gpu, d), xg, min_nn_count=1)
        g2 = sdf_cpu.get_gradient(xg, s2)
        second = torch.autograd.grad(((g2.norm(dim=-1) - 1.0) ** 2).mean() + s2.abs().mean(), [feats] + P)
        small = [hnp.sdf_fused(gpu, _Dec({**dec}), xc[:nb], need_grad=True, need_std=True) for nb in (1, 2, 3, 5)]
        res[mode] = (out, s.detach(), first, second, small)
        errs[mode] = dict(sdf=rel_err(out[0], ref["sdf"]), grad=rel_err(out[1], ref["grad"]),
                          std=rel_err(out[4], ref["std"]) if not weighted_first else float(out[4].abs().max()),
                          train_sdf=rel_err(s, ref["sdf"]), grad2_x=rel_err(g2, ref["grad"]),
                          **{"d1_" + n: rel_err(a.reshape(b.shape), b) for n, a, b in zip(names, first, ref["first"])},
                          **{"d2_" + n: rel_err(a.reshape(b.shape), b) for n, a, b in zip(names, second, ref["second"])})
    if family == MATRIX:
        a, b = res["mfma"], res["vector"]
        errs["families"] = dict(sdf=rel_err(a[0][0], b[0][0]), grad=rel_err(a[0][1], b[0][1]),
                                std=rel_err(a[0][4], b[0][4]), train_sdf=rel_err(a[1], b[1]),
                                **{"d1_" + n: rel_err(u, v) for n, u, v in zip(names, a[2], b[2])})
    print(f"F={F} H={H} nn_k={nn_k} weighted_first={weighted_first}: {errs}")
    for mode, (out, _, _, _, small) in res.items():
        assert torch.equal(out[2].cpu(), ref["cnt"])
        assert all(v <= 1e-4 for v in errs[mode].values()), (mode, errs[mode])
        # every fill level of the last four-query wave step: a query's result does not depend on its batch
        for nb, sm in zip((1, 2, 3, 5), small):
            for u, v in zip(sm, out):
                assert u is None and v is None or torch.equal(u, v[:nb]), (mode, nb)
    if family == MATRIX:
        assert torch.equal(res["mfma"][0][2], res["vector"][0][2])
        e = errs["families"]
        assert max(e["sdf"], e["grad"], e["std"], e["train_sdf"]) <= 2e-5, e
        assert all(e["d1_" + n] <= 5e-5 for n in names), e
