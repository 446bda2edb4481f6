"""Semantic loss block (pings_amd.semantic_losses, csrc/sem_loss.hip) against the fp64 restatement of
utils/mapper.py:863-866 / 929-946 (tests/sem_ref.py)."""
import math
from types import SimpleNamespace as NS

import pytest
import torch

import abi_header as hdr
import sem_ref
from conftest import rel_err

TOL = 1e-4                 # the project's tolerance for the neighbouring block (tests/test_sdf_losses.py)


# ------------------------------------------------------------------ CPU
def _seven_rows():
    """Seven rows, two neighbours, three classes.  Neighbour 0 of row b has probabilities P[b % 3], neighbour 1 has
    P[(b + 1) % 3], with P[i] = 1/2 at class i and 1/4 elsewhere; the logits are log P plus a shift per vector, so every
    log-softmax value is -ln 2 or -2 ln 2.  Weights (1/4, 3/4)."""
    P = torch.full((3, 3), 0.25, dtype=torch.float64) + 0.25 * torch.eye(3, dtype=torch.float64)
    raw = torch.stack([torch.stack([P[b % 3].log() + 0.3 * b, P[(b + 1) % 3].log() - 1.7 * b]) for b in range(7)])
    w = torch.tensor([0.25, 0.75], dtype=torch.float64).repeat(7, 1)
    y = torch.tensor([0, 2, -1, 1, 1, 0, 2])
    return raw, w, y


def test_restatement_matches_hand_computed_case():
    # per-row sum_j w_j log p_j[y] in units of ln 2: rows 0..6 = -1.75, -1.25, (unlabelled), -1.25, -1.75, -1.25, -2
    raw, w, y = _seven_rows()
    ln2 = math.log(2.0)
    # labels > 0: rows 1, 3, 4, 6; every 2nd: rows 1, 4
    assert float(sem_ref.nll(raw, w, y, False, 2)) == pytest.approx(1.5 * ln2, rel=1e-12)
    assert sem_ref.selected_rows(y, False, 2).tolist() == [1, 4]
    # labels >= 0: rows 0, 1, 3, 4, 5, 6; every 3rd: rows 0, 4
    assert float(sem_ref.nll(raw, w, y, True, 3)) == pytest.approx(1.75 * ln2, rel=1e-12)
    assert sem_ref.selected_rows(y, True, 3).tolist() == [0, 4]
    assert float(sem_ref.nll(raw, w, y, False, 1)) == pytest.approx(6.25 / 4 * ln2, rel=1e-12)
    # weighted_first: one vector per row, weights one
    assert float(sem_ref.nll(raw[:, 0], None, y, False, 2)) == pytest.approx(1.5 * ln2, rel=1e-12)   # rows 1, 4: -2, -1


def test_restatement_empty_selection_is_nan():
    raw, w, y = _seven_rows()
    assert math.isnan(float(sem_ref.nll(raw, w, torch.full_like(y, -1), True, 2)))
    assert math.isnan(float(sem_ref.nll(raw, w, torch.zeros_like(y), False, 1)))


def test_header_declares_the_semantic_loss_symbols():
    names = hdr.header_symbols()
    for n in ("pings_sem_loss_scratch_bytes", "pings_sem_loss_forward", "pings_sem_loss_backward"):
        assert n in names
    assert "pings_sem_loss_args" in hdr.structs()


def test_argument_validation():
    from pings_amd import _lib
    from pings_amd.semantic_losses import semantic_loss, semantic_nll

    raw, w, y = (t.float() if t.is_floating_point() else t for t in _seven_rows())
    with pytest.raises(_lib.PingsHipError, match="HIP device only"):
        semantic_nll(raw, w, y)
    with pytest.raises(ValueError, match="raw"):
        semantic_nll(raw[:, 0], w, y)
    with pytest.raises(ValueError, match="raw"):
        semantic_nll(raw, None, y)
    with pytest.raises(ValueError, match="w must be"):
        semantic_nll(raw, w[:, :1], y)
    with pytest.raises(ValueError, match="sem_label"):
        semantic_nll(raw, w, y[:-1])
    with pytest.raises(TypeError, match="raw"):
        semantic_nll(raw.double(), w, y)
    with pytest.raises(TypeError, match="w must be"):
        semantic_nll(raw, w.double(), y)
    with pytest.raises(TypeError, match="sem_label"):
        semantic_nll(raw, w, y.float())
    with pytest.raises(ValueError, match="decimation"):
        semantic_nll(raw, w, y, decimation=0)

    cfg = NS(weighted_first=False, freespace_label_on=False, sem_label_decimation=2)
    geo = torch.zeros(7, 2, 5)
    with pytest.raises(ValueError, match="sem_mlp"):
        semantic_loss(NS(config=cfg, sem_mlp=None), geo, w, y)
    dec = NS(layers=[NS(weight=torch.zeros(64, 5), bias=torch.zeros(64))],
             lout=NS(weight=torch.zeros(3, 64), bias=torch.zeros(3)), use_leaky_relu=False)
    m = NS(config=cfg, sem_mlp=dec)
    with pytest.raises(ValueError, match="geo_feature"):
        semantic_loss(m, geo[:, 0], w, y)
    with pytest.raises(_lib.PingsHipError, match="HIP device only"):
        semantic_loss(m, geo, w, y)
    cfg.sem_label_decimation = 0
    with pytest.raises(ValueError, match="sem_label_decimation"):
        semantic_loss(m, geo, w, y)


# ------------------------------------------------------------------ GPU, block level
def _inputs(B, k, S, seed=0, scale=1.0, wf=False):
    """raw, w (None for weighted_first), labels from {-1, 0, 1..S-1} (CPU; the weights sum to one per row)."""
    g = torch.Generator().manual_seed(seed)
    raw = scale * torch.randn((B, S) if wf else (B, k, S), generator=g)
    w = None if wf else torch.softmax(torch.randn(B, k, generator=g), dim=1)
    y = torch.randint(-1, S, (B,), generator=g, dtype=torch.int32)
    return raw, w, y


def _hip(raw, w, y, fs, d, g=1.0):
    from pings_amd.semantic_losses import semantic_nll

    x = raw.cuda().requires_grad_(True)
    R = semantic_nll(x, None if w is None else w.cuda(), y.cuda(), freespace_label_on=fs, decimation=d)
    (dx,) = torch.autograd.grad(g * R.nll, x)
    return R, dx


def _ref(raw, w, y, fs, d, g=1.0):
    x = raw.double().requires_grad_(True)
    v = sem_ref.nll(x, None if w is None else w.double(), y.long(), fs, d)
    (dx,) = torch.autograd.grad(g * v, x)
    return v.detach(), dx


def _check(raw, w, y, fs, d, g=1.0):
    R, dx = _hip(raw, w, y, fs, d, g)
    v, dr = _ref(raw, w, y, fs, d, g)
    want = sem_ref.selected_rows(y.long(), fs, d)
    assert torch.equal(torch.nonzero(R.selected.cpu()).view(-1), want)
    assert float(R.counts[0]) == len(want) and float(R.counts[1]) == 0
    assert R.nll.dim() == 0 and R.nll.grad_fn is not None
    e_v, e_g = rel_err(R.nll, v), rel_err(dx, dr)
    print(f"B={raw.shape[0]} shape={tuple(raw.shape)} d={d} n={len(want)}: rel_err value {e_v:.3g} d_raw {e_g:.3g}")
    assert len(want) > 0 and float(dr.abs().max()) > 0
    assert e_v <= TOL and e_g <= TOL
    unsel = ~R.selected
    assert float(dx[unsel].abs().max() if bool(unsel.any()) else 0.0) == 0.0      # exactly zero off the selection
    return R, dx


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_values_and_gradient_match_fp64_restatement_over_batch_sizes(B):
    raw, w, y = _inputs(B, 6, 21, seed=B)
    if B == 1:
        y[0] = 5                                    # the one row is labelled
    _check(raw, w, y, False, 3, g=0.7)


@pytest.mark.gpu
@pytest.mark.parametrize("wf", [False, True])
@pytest.mark.parametrize("k,S", [(1, 2), (16, 32), (6, 21)])
def test_values_and_gradient_match_fp64_restatement_over_shapes(k, S, wf):
    raw, w, y = _inputs(517, k, S, seed=10 * k + S, wf=wf)
    _check(raw, w, y, True, 3)
    _check(raw, w, y, False, 1)


@pytest.mark.gpu
def test_large_logits_need_the_max_subtraction():
    raw, w, y = _inputs(300, 6, 21, seed=3)
    raw = 80.0 * (2.0 * torch.rand(raw.shape, generator=torch.Generator().manual_seed(4)) - 1.0)
    assert float(raw.max()) > 75 and float(raw.min()) < -75          # exp() of these overflows fp32 without it
    R, _ = _check(raw, w, y, False, 1)
    assert bool(torch.isfinite(R.nll))


@pytest.mark.gpu
def test_a_row_whose_weights_are_all_zero():
    raw, w, y = _inputs(200, 6, 21, seed=5)
    y[7] = 3
    w[7] = 0.0
    R, dx = _check(raw, w, y, False, 1)
    assert bool(R.selected[7]) and float(dx[7].abs().max()) == 0.0


def _labels(case, B, S, fs, seed=11):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(-1, S, (B,), generator=g, dtype=torch.int32)
    if case == "none":
        y = torch.full_like(y, -1) if fs else torch.randint(-1, 1, (B,), generator=g, dtype=torch.int32)
    elif case == "fewer_than_d":
        y = torch.full_like(y, -1)
        y[[17, 200, 250]] = torch.tensor([4, 1, S - 1], dtype=torch.int32)
    elif case == "all":
        y = torch.randint(1, S, (B,), generator=g, dtype=torch.int32)
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("fs", [False, True])
@pytest.mark.parametrize("d", [4, 1])
@pytest.mark.parametrize("case", ["none", "fewer_than_d", "not_multiple", "all"])
def test_selection_is_nonzero_decimated(case, d, fs):
    B, k, S = 301, 6, 21
    raw, w, _ = _inputs(B, k, S, seed=12)
    y = _labels(case, B, S, fs)
    mask = (y >= 0) if fs else (y > 0)
    M = int(mask.sum())
    want = torch.nonzero(mask).view(-1)[::d]
    if case == "not_multiple":
        if d > 1 and M % d == 0:                   # drop one labelled row so that M is no multiple of d
            y[int(torch.nonzero(mask)[0])] = -1
            mask = (y >= 0) if fs else (y > 0)
            M = int(mask.sum())
            want = torch.nonzero(mask).view(-1)[::d]
        assert d == 1 or M % d != 0
    if case == "fewer_than_d":
        assert M == 3
    if case == "all":
        assert M == B
    R32, d32 = _hip(raw, w, y, fs, d)
    R64, d64 = _hip(raw, w, y.long(), fs, d)
    assert torch.equal(torch.nonzero(R32.selected.cpu()).view(-1), want)
    assert R32.selected.dtype == torch.bool and R32.selected.shape == (B,)
    assert float(R32.counts[0]) == len(want) == (M + d - 1) // d
    # int32 and int64 labels: the same bits
    assert torch.equal(R32.selected, R64.selected) and torch.equal(d32, d64)
    assert torch.equal(R32.nll.view(torch.int32), R64.nll.view(torch.int32))
    if case == "none":
        assert M == 0 and bool(torch.isnan(R32.nll))
        assert float(d32.abs().max()) == 0.0 and not bool(torch.isnan(d32).any())
    else:
        v, dr = _ref(raw, w, y, fs, d)
        assert rel_err(R32.nll, v) <= TOL and rel_err(d32, dr) <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 3])
def test_out_of_range_labels_are_counted_and_unlabelled(d):
    B, k, S = 301, 6, 21
    raw, w, y = _inputs(B, k, S, seed=13)
    bad = [0, 150, 299]                            # not the last row
    y_bad = y.clone()
    y_bad[bad] = torch.tensor([S, S + 5, 2 ** 31 - 1], dtype=torch.int32)
    y_ref = y.clone()
    y_ref[bad] = -1
    for lab in (y_bad, y_bad.long()):
        R, dx = _hip(raw, w, lab, True, d)
        assert float(R.counts[1]) == 3
        assert not bool(R.selected[bad].any())
        assert torch.equal(torch.nonzero(R.selected.cpu()).view(-1), sem_ref.selected_rows(y_ref.long(), True, d))
        v, dr = _ref(raw, w, y_ref, True, d)
        assert rel_err(R.nll, v) <= TOL and rel_err(dx, dr) <= TOL
        assert float(dx[bad].abs().max()) == 0.0


@pytest.mark.gpu
def test_argument_limits_are_status_codes():
    import ctypes as C

    from pings_amd import _abi, _lib
    from pings_amd.semantic_losses import semantic_nll

    L = _lib.lib()
    for k, S, msg in ((17, 21, b"k must be"), (6, 33, b"S must be")):
        raw, w, y = (t.cuda() for t in _inputs(8, k, S))
        sel = torch.zeros(8, dtype=torch.bool, device="cuda")
        scr = torch.zeros(int(L.pings_sem_loss_scratch_bytes(8)) // 8, dtype=torch.float64, device="cuda")
        out = torch.zeros(3, dtype=torch.float64, device="cuda")
        a = _abi.SemLossArgs(8, k, S, 1, 0, raw.data_ptr(), w.data_ptr(), y.data_ptr(), sel.data_ptr(),
                             scr.data_ptr(), out[2:].data_ptr(), out.data_ptr())
        assert L.pings_sem_loss_forward(C.byref(a), None) == 1
        assert msg in L.pings_last_error()
        with pytest.raises(_lib.PingsHipError, match=msg.decode()):
            semantic_nll(raw, w, y)
    assert L.pings_sem_loss_scratch_bytes(0) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 3])
def test_two_runs_give_the_same_bits(d):
    raw, w, y = _inputs(4097, 6, 21, seed=14)
    R1, g1 = _hip(raw, w, y, False, d)
    R2, g2 = _hip(raw, w, y, False, d)
    assert torch.equal(R1.nll.view(torch.int32), R2.nll.view(torch.int32))
    assert torch.equal(g1, g2) and torch.equal(R1.selected, R2.selected) and torch.equal(R1.counts, R2.counts)


# ------------------------------------------------------------------ GPU, end to end
SEM_W, N_CLASSES = 0.7, 21


def _sem_params(st, seed=9, H=64, S=N_CLASSES):
    from test_sdf_losses import _dec_params

    g = torch.Generator().manual_seed(seed)
    IN = int(_dec_params(st)[0].shape[1])
    return [0.4 * torch.randn(H, IN, generator=g), 0.1 * torch.randn(H, generator=g),
            0.3 * torch.randn(S, H, generator=g), 0.1 * torch.randn(S, generator=g)]


def _sem_mapper(st, fs, d=3):
    from test_sdf_losses import _cfg, _gpu_mapper

    m = _gpu_mapper(st, _cfg(st, d=3, freespace_label_on=fs, sem_label_decimation=d))
    p = [torch.nn.Parameter(t.clone().cuda()) for t in _sem_params(st)]
    m.sem_mlp = NS(layers=[NS(weight=p[0], bias=p[1])], lout=NS(weight=p[2], bias=p[3]), use_leaky_relu=False)
    return m, p


def _sem_labels(B, seed=21):
    return torch.randint(-1, N_CLASSES, (B,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)


def _ref_total(st, ins, y, fs, d):
    """fp64: BCE + SEM_W * nll on one query, and its gradients w.r.t. the geo table and the semantic decoder."""
    import sdf_losses_ref as ref
    from oracle import sdf_cpu
    from test_sdf_losses import _cfg, _dec_params, _sigma

    coord, label, ts, weight, _ = ins
    cfg = _cfg(st, d=3)
    geo = torch.as_tensor(st["local_geo_features"]).double().requires_grad_(True)
    sp = [p.double().requires_grad_(True) for p in _sem_params(st)]
    npm = ref.map64(st, geo)
    dec = sdf_cpu.MLP(*[p.double() for p in _dec_params(st)], float(st["sdf_scale"]))
    bce = ref.block(cfg, _sigma(st), npm, dec, None, coord.double(), label.double(), ts, weight.double(),
                    eikonal=False)[0]
    geo_feature, _, weight_knn, _, _ = npm.query_feature(coord.double(), ts, accumulate_stability=False)
    raw = sdf_cpu.MLP(*sp).mlp(geo_feature)
    nll = sem_ref.nll(raw, None if npm.weighted_first else weight_knn, y.long(), fs, d)
    grads = torch.autograd.grad(bce + SEM_W * nll, [geo] + sp)
    return nll.detach(), grads


@pytest.mark.gpu
@pytest.mark.parametrize("fs", [False, True])
@pytest.mark.parametrize("name", ["gs_f32", "pin_f8"])
def test_end_to_end_matches_fp64_restatement(name, fs):
    from pings_amd.sdf_losses import sdf_losses
    from pings_amd.semantic_losses import semantic_loss
    from test_sdf_losses import _batch, _state

    st = _state(name)
    ins = _batch(st, B=600, seed=1)
    y = _sem_labels(600)
    m, sp = _sem_mapper(st, fs)
    coord, label, ts, weight, _ = (t.cuda() for t in ins)
    S = sdf_losses(m, coord, label, ts, weight, eikonal=False)
    R = semantic_loss(m, S.query[0], S.query[2], y.cuda())
    total = S.bce + SEM_W * R.nll
    gh = torch.autograd.grad(total, [m.neural_points.local_geo_features] + sp)
    v, gr = _ref_total(st, ins, y, fs, 3)
    assert float(R.counts[0]) == len(sem_ref.selected_rows(y.long(), fs, 3)) > 10
    print(f"{name} fs={fs}: nll {float(R.nll.detach()):.6f} ref {float(v):.6f} rel_err {rel_err(R.nll, v):.3g}")
    assert rel_err(R.nll, v) <= TOL
    for n, a, b in zip(("local_geo_features", "sem.W1", "sem.b1", "sem.W2", "sem.b2"), gh, gr):
        e = rel_err(a.reshape(b.shape), b)
        print(f"  d {n}: rel_err {e:.3g}")
        assert float(b.abs().max()) > 0, n
        assert e <= TOL, (n, e)


@pytest.mark.gpu
def test_no_host_waits_and_no_growth():
    import gc

    from pings_amd import _lib
    from pings_amd.sdf_losses import sdf_losses
    from pings_amd.semantic_losses import semantic_loss
    from test_sdf_losses import _batch, _params, _state

    st = _state("gs_f32")
    m, sp = _sem_mapper(st, False)
    coord, label, ts, weight, cl = (t.cuda() for t in _batch(st, B=600, seed=6))
    y = _sem_labels(600).cuda()
    params = _params(m) + sp
    cert0 = m.neural_points.local_point_certainties.clone()

    def step():
        m.neural_points.local_point_certainties.copy_(cert0)
        S = sdf_losses(m, coord, label, ts, weight, cl, eikonal=True, color=True)
        R = semantic_loss(m, S.query[0], S.query[2], y)
        tot = S.bce + 0.5 * S.eikonal + 0.8 * S.color + SEM_W * R.nll
        return [R.nll.detach().clone(), R.counts.clone(), R.selected.clone()], torch.autograd.grad(tot, params)

    step()                                       # first query of the map builds its search index (cached)
    torch.cuda.synchronize()
    _lib.sync_counts(reset=True)
    probe = torch.ones(1, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):        # positive control: the mode catches a device-to-host read
            probe.sum().item()
        v1, g1 = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert _lib.sync_counts() == {}
    v2, g2 = step()
    for x, z in zip(v1 + list(g1), v2 + list(g2)):
        assert torch.equal(x, z)
    gc.disable()
    try:
        step()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() <= base
    finally:
        gc.enable()
