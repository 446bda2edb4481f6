"""The colour branches of the device-resident odometry loop (install(..., loop=True, colour=True): SDF forward with its
neighbour rows out, `pings_color_forward`, `pings_reg_assemble_color`, the unchanged `pings_reg_step`) against the
reference's own runs (tests/golden/tracking_colour_{photo,consist}.npz, tools/make_tracking_colour_golden.py), the fp64
restatement (tests/tracking_colour_ref.py) and, through the C ABI with hand-made arrays, the fp64 sums with the bound
derived in that module (28 fp32 roundings of a sum's magnitude sum, 5 for photo_part)."""
import ctypes as C
import functools
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import tracker_edges_ref as E
import tracking_colour_ref as cref
import tracking_ref as ref
from test_tracking import TOL_ROT, TOL_T, _cfg, _fake_module, _rot_err

GOLDEN = Path(__file__).parent / "golden"
FIXTURES = ["photo", "consist"]
U, EPS = 2.0 ** -24, 2.0 ** -52
LAM = E.f32(0.7)                              # photo_weight of the assemble tests, an fp32 number
ASSEMBLE_N = (9, 10, 65537)                   # below / at the 10-valid-point rule; a second grid-stride pass
ASSEMBLE_CASES = [(n, mode, ch) for n in ASSEMBLE_N for mode in (cref.PHOTO, cref.CONSIST) for ch in (1, 3)]


@functools.lru_cache(maxsize=None)
def _fix(name):
    z = np.load(GOLDEN / f"tracking_colour_{name}.npz")
    return {k: z[k] for k in z.files}


def _colour_cfg(st, **kw):
    return _cfg(st, color_on=bool(st["cfg.color_on"]), **kw)


@functools.lru_cache(maxsize=None)
def _assemble_case(n, mode, ch):
    """(inputs, colours, settings, fp64 restatement): shared by the CPU and the device tests, never modified."""
    inp = E.make_inputs(n, 4000 + 7 * n + 3 * mode + ch, offset=0.0, label_nonzero=True, all_valid=n < 64)
    st = dict(E.settings("all"))
    col = cref.make_colours(inp, ch, seed=n + mode + ch)
    valid = E.assemble(inp, st).valid.numpy()
    cref.poison_invalid(col, valid)
    return inp, col, st, cref.assemble_colour(inp, col, st, mode, LAM)


def _ratio(err, bound):
    err, bound = np.asarray(err, np.float64).ravel(), np.asarray(bound, np.float64).ravel()
    assert np.all(err[bound == 0] == 0), "an entry without any contribution is not exactly zero"
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference_colour_runs(name):
    st = _fix(name)
    cfg = _colour_cfg(st)
    assert cfg.color_on and cfg.color_channel == 3 and (cfg.photometric_loss_on or cfg.consist_wieght_on)
    npm, dec = ref.cpu_map(st)
    q = cref.cpu_query(npm, dec, cref.cpu_colour_decoder(st), int(cfg.infer_bs), int(cfg.track_mask_query_nn_k),
                       want_jac=bool(cfg.photometric_loss_on))
    src, col = torch.as_tensor(st["src"]).double(), torch.as_tensor(st["src_color"]).double()
    T, valid, trace, photo = cref.tracking(q, ref.cpu_solve, cfg, src, torch.as_tensor(st["init_pose"]), col)
    assert len(trace) == int(st["iterations"]) and valid == bool(st["valid_flag"])
    for i, (dT, cnt, res) in enumerate(trace):
        er, et = _rot_err(dT, st["delta"][i])
        assert er <= TOL_ROT and et <= TOL_T, (i, er, et)
        assert abs(cnt - int(st["count"][i])) <= max(2, 1e-3 * cnt), (i, cnt, st["count"][i])
        assert abs(res - float(st["residual"][i])) <= 1e-3 * max(1.0, abs(float(st["residual"][i]))), i
        if cfg.photometric_loss_on:
            assert abs(photo[i] - float(st["photo_residual"][i])) <= 1e-3 * float(st["photo_residual"][i]), i
        else:
            assert photo[i] is None and np.isnan(st["photo_residual"][i])
    er, et = _rot_err(T, st["T"])
    assert er <= TOL_ROT and et <= TOL_T
    # the colour term is present: the recorded first step is not the geometry-only one
    assert float(st["first_step_shift"]) >= 10 * TOL_T
    assert _rot_err(st["delta"][0], st["geo_first_delta"])[1] >= 10 * TOL_T


@pytest.mark.parametrize("branch", ["photometric_loss_on", "consist_wieght_on"])
def test_colour_option_raises_on_host_tensors_and_the_default_install_turns_it_off(branch):
    from pings_amd import _lib, tracker_ops as TO

    m, calls = _fake_module()
    TO.install(m, loop=True, colour=True)
    try:
        cfg = _cfg(_fix("photo"), color_on=True, **{"photometric_loss_on": False, "consist_wieght_on": False,
                                                    branch: True})
        self = m.Tracker()
        self.config = cfg
        src, col = torch.rand(50, 3), torch.rand(50, 3)
        with pytest.raises(_lib.PingsHipError):
            self.tracking(src, None, col)
        with pytest.raises(_lib.PingsHipError):
            self.registration_step(src, None, torch.zeros(50), col, 0.4, 2.5)
        assert calls == []
        TO.install(m, loop=True)
        assert self.tracking(src, None, col) == "orig-tracking"
        assert self.registration_step(src, None, torch.zeros(50), col, 0.4, 2.5) == "orig-step"
        assert [c[0] for c in calls] == ["tracking", "registration_step"]
    finally:
        TO.install(m, loop=True)
        TO._ORIG.clear()


def test_new_symbols_are_declared_in_the_header_and_mirrored():
    import abi_header
    from pings_amd import _abi

    syms, structs, defines = set(abi_header.header_symbols()), abi_header.structs(), abi_header.defines()
    assert {"pings_color_forward", "pings_reg_assemble_color"} <= syms
    assert "pings_color_forward" in _abi.SIGNATURES and "pings_reg_assemble_color" in _abi.SIGNATURES
    assert [n for _, n in structs["pings_reg_color_args"]] == ["src_color", "color_pred", "color_jac", "channels",
                                                               "mode", "photo_weight", "photo_part"]
    assert "pings_color_decoder" in structs
    assert defines["PINGS_REG_COLOR_PHOTO"] == _abi.REG_COLOR_PHOTO == cref.PHOTO
    assert defines["PINGS_REG_COLOR_CONSIST"] == _abi.REG_COLOR_CONSIST == cref.CONSIST
    assert defines["PINGS_ABI_VERSION"] == 11
    # the layout the existing kernels read is untouched
    assert [n for _, n in structs["pings_reg_loop_args"]] == [f[0] for f in _abi.RegLoopArgs._fields_]


@pytest.mark.parametrize("n,mode,ch", ASSEMBLE_CASES)
def test_fp32_restatement_is_within_a_quarter_of_the_colour_assemble_bound(n, mode, ch):
    inp, col, st, want = _assemble_case(n, mode, ch)
    f32 = cref.assemble_colour(inp, col, st, mode, LAM, torch.float32)
    assert torch.equal(f32.valid, want.valid) and f32.count == want.count
    assert want.count == n if n < 64 else 0.2 * n < want.count < 0.7 * n
    ratio = _ratio(np.abs(E.totals(f32) - E.totals(want)), cref.COLOUR_ROUNDINGS * U * E.total_bounds(want))
    rp = abs(f32.photo - want.photo) / (cref.PHOTO_PART_ROUNDINGS * U * want.photo_mag)
    print(f"\n[n={n} mode={mode} C={ch}] valid {want.count}  fp32 error / bound {ratio:.3f}  photo_part {rp:.3f}")
    assert ratio <= 0.25 and rp <= 0.25
    if want.count >= 10:        # the step behind it solves a system that fp32 rounding does not decide
        assert E.step(E.normal_eq_from_totals(E.totals(f32), True), st["lm_lambda"]).cond <= 1e6
    # the colour terms are in the sums: they differ from the geometric assemble's by far more than the bound
    geo = E.assemble(inp, st)
    assert np.abs(E.totals(want) - E.totals(geo))[:27].max() > 1e3 * U * np.abs(E.totals(geo))[:27].max()


# ------------------------------------------------------------------ GPU: pings_reg_assemble_color through the C ABI
@pytest.mark.gpu
@pytest.mark.parametrize("n,mode,ch", ASSEMBLE_CASES)
def test_assemble_color_matches_fp64_and_the_step_solves_its_system(n, mode, ch):
    """valid[n] and the count exactly, every sum within 28 u (+ n 2^-52) of its magnitude sum, photo_part within 5 u;
    slot 31 stays 0; two launches bit-equal; then `pings_reg_step` on those partials: the identity below 10 valid
    points, else the fp64 solve of the kernel's own system."""
    from pings_amd import _abi
    from test_tracker_edges import _Dev, _bits, _up

    inp, col, st, want = _assemble_case(n, mode, ch)
    st = dict(st, flags=st["flags"] | E.F_WEIGHTED)
    pose = np.eye(4)
    dev = _Dev(inp, st, pose)
    bufs = [_up(col.src, n), _up(col.pred, n), _up(col.jac, n)]
    photo_part = torch.full((dev.nb,), -7.0, dtype=torch.float64, device="cuda")
    ca = _abi.RegColorArgs(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr() if mode == cref.PHOTO else None,
                           ch, mode, LAM, photo_part.data_ptr())

    def run():
        dev.part.fill_(-7.0)
        photo_part.fill_(-7.0)
        rc = dev.L.pings_reg_assemble_color(C.byref(dev.a), C.byref(ca), dev.stream)
        assert rc == 0, dev.L.pings_last_error()
        return dev.partials().copy(), photo_part.cpu().numpy().copy()

    first, photo = run()
    got_valid = dev.valid.cpu().numpy()[:n].astype(bool)
    assert np.array_equal(got_valid, want.valid.numpy())
    tot = dev.totals()
    assert tot[27] == want.count and tot[31] == 0.0 and np.isfinite(tot).all()
    per_term = cref.COLOUR_ROUNDINGS * U + n * EPS
    ratio = _ratio(np.abs(tot - E.totals(want)), per_term * E.total_bounds(want))
    ps = float(np.sum(photo))
    rp = abs(ps - want.photo) / ((cref.PHOTO_PART_ROUNDINGS * U + n * EPS) * want.photo_mag)
    print(f"\n[n={n} mode={mode} C={ch}] valid {want.count}  error / bound {ratio:.3f}  photo_part {rp:.3f}")
    assert ratio <= 1.0 and rp <= 1.0
    again, photo2 = run()
    assert np.array_equal(_bits(first), _bits(again)) and np.array_equal(_bits(photo), _bits(photo2))
    # the unchanged step behind the new assemble
    dev.call("step")
    delta = dev.delta.cpu().numpy()
    cnt, status, vals = dev.host_record()
    assert cnt == want.count
    if want.count < 10:
        assert np.array_equal(_bits(delta), _bits(np.eye(4))) and np.array_equal(_bits(vals), np.zeros(3, np.int64))
        return
    s = E.step(E.normal_eq_from_totals(tot, True), st["lm_lambda"], pose)
    bd = np.full((4, 4), E.solve_tolerance(s.cond) * np.abs(s.t).max() + 16 * EPS)
    bd[3] = 0.0
    r1 = _ratio(np.abs(delta - s.dT), bd)
    print(f"  cond {s.cond:.3g}  delta error / bound {r1:.3g}")
    assert r1 <= 1.0 and status == 0
    assert vals[0] == float(np.float32(tot[29] / tot[27])) * 100.0


@pytest.mark.gpu
def test_assemble_color_rejects_bad_arguments():
    from pings_amd import _abi
    from test_tracker_edges import _Dev

    inp, col, st, _ = _assemble_case(10, cref.PHOTO, 3)
    dev = _Dev(inp, st)
    pp = torch.zeros(dev.nb, dtype=torch.float64, device="cuda")
    ok = lambda **kw: _abi.RegColorArgs(**{**dict(src_color=pp.data_ptr(), color_pred=pp.data_ptr(),
                                                  color_jac=pp.data_ptr(), channels=3, mode=cref.PHOTO,
                                                  photo_weight=LAM, photo_part=pp.data_ptr()), **kw})
    for bad in (ok(channels=2), ok(mode=0), ok(color_jac=None), ok(photo_part=None), ok(src_color=None)):
        assert dev.L.pings_reg_assemble_color(C.byref(dev.a), C.byref(bad), dev.stream) == 1
    assert dev.L.pings_reg_assemble_color(C.byref(dev.a), None, dev.stream) == 1


# ------------------------------------------------------------------ GPU: the loop against the golden runs
def _tracker(st, cfg):
    from test_color_query_edges import _ColourDec
    from test_tracking import _tracker as geo_tracker

    trk = geo_tracker(st, cfg)
    trk.color_mlp = _ColourDec({k: st[k] for k in st if k.startswith("cdec.")})
    return trk


@pytest.fixture
def colour_loop():
    from pings_amd import tracker_ops as TO

    m, calls = _fake_module()
    TO.install(m, loop=True, colour=True)
    yield TO, calls
    TO.install(m, loop=True)
    TO._ORIG.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_hip_colour_tracking_matches_the_reference_runs(name, colour_loop):
    TO, calls = colour_loop
    st = _fix(name)
    trk = _tracker(st, _colour_cfg(st))
    src, col = torch.as_tensor(st["src"]).cuda(), torch.as_tensor(st["src_color"]).cuda()
    init = torch.as_tensor(st["init_pose"]).cuda()
    T, cov, wpc, valid = TO.tracking(trk, src, init, source_colors=col)
    tr = TO.last_trace.cpu()
    assert calls == [] and cov is None and wpc is None
    assert tr.shape[0] == int(st["iterations"]) and valid == bool(st["valid_flag"])
    for i in range(tr.shape[0]):
        er, et = _rot_err(tr[i, 8:].view(4, 4), st["delta"][i])
        print(f"\n[{name} it {i}] rot err {er:.3g} rad  tran err {et:.3g} m")
        assert er <= TOL_ROT and et <= TOL_T, (i, er, et)
        assert abs(int(tr[i, 0]) - int(st["count"][i])) <= max(2, 1e-3 * float(tr[i, 0])), i
        assert abs(float(tr[i, 1]) - float(st["residual"][i])) <= 1e-3 * max(1.0, float(st["residual"][i])), i
    er, et = _rot_err(T, st["T"])
    assert er <= TOL_ROT and et <= TOL_T
    from pings_amd import _lib

    with pytest.raises(_lib.PingsHipError):           # colours on the host: no CPU path
        TO.tracking(trk, src, init, source_colors=col.cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_hip_colour_registration_step_matches_the_first_iteration(name, colour_loop):
    TO, calls = colour_loop
    st = _fix(name)
    cfg = _colour_cfg(st)
    trk = _tracker(st, cfg)
    src, col = torch.as_tensor(st["src"]).cuda(), torch.as_tensor(st["src_color"]).cuda()
    cur = ref.transform(src, torch.as_tensor(st["init_pose"]).cuda())
    out = TO.registration_step(trk, cur, None, torch.zeros(src.shape[0], device="cuda"), col, cfg.reg_min_grad_norm,
                               cfg.reg_max_grad_norm, cfg.reg_GM_dist_m, cfg.reg_GM_grad, cfg.reg_lm_lambda)
    assert calls == [] and len(out) == 7 and out[1] is None and out[2] is None and out[3] is None
    er, et = _rot_err(out[0], st["delta"][0])
    assert er <= TOL_ROT and et <= TOL_T
    assert abs(out[5] - float(st["residual"][0])) <= 1e-3 * float(st["residual"][0])
    assert abs(out[4].shape[0] - int(st["count"][0])) <= 2
    if cfg.photometric_loss_on:
        want = float(st["photo_residual"][0])
        assert isinstance(out[6], float) and abs(out[6] - want) <= 1e-3 * want
    else:
        assert out[6] is None


@pytest.mark.gpu
def test_hip_colour_tracking_reads_the_host_once_per_iteration_and_is_deterministic(colour_loop):
    from pings_amd import _lib

    TO, _ = colour_loop
    st = _fix("photo")
    trk = _tracker(st, _colour_cfg(st))
    src, col = torch.as_tensor(st["src"]).cuda(), torch.as_tensor(st["src_color"]).cuda()
    init = torch.as_tensor(st["init_pose"]).cuda()
    TO.tracking(trk, src, init, source_colors=col)     # warm-up: first-use allocations and reads of the map
    torch.cuda.synchronize()
    _lib.sync_counts(reset=True)
    torch.cuda.set_sync_debug_mode("error")
    try:
        T1, _, _, v1 = TO.tracking(trk, src, init, source_colors=col)
        tr1 = TO.last_trace
    finally:
        torch.cuda.set_sync_debug_mode(0)
    counts = _lib.sync_counts(reset=True)
    assert counts == {"tracking_iteration": tr1.shape[0]}
    T2, _, _, v2 = TO.tracking(trk, src, init, source_colors=col)
    assert torch.equal(T1, T2) and v1 == v2 and torch.equal(tr1, TO.last_trace)


@pytest.mark.gpu
def test_query_source_points_colour_branch_matches_the_restatement_and_keeps_the_composed_path():
    from pings_amd import neural_points as hnp, tracker_ops as TO
    from test_color_query_edges import _ColourDec, _gate

    st = _fix("photo")
    cfg = _colour_cfg(st)
    trk = _tracker(st, cfg)
    cur = ref.transform(torch.as_tensor(st["src"]), torch.as_tensor(st["init_pose"])).float()
    npm, _ = ref.cpu_map(st)
    want = cref.colour_query(npm, cref.cpu_colour_decoder(st), cur.double())
    out = TO.query_source_points(trk, cur.cuda(), 1024, True, True, True, True, query_locally=True,
                                 mask_min_nn_count=int(cfg.track_mask_query_nn_k))
    keep = ~want.flagged
    assert float((~keep).double().mean()) <= cref.KINK_CAP
    for got, w, k in ((out[2], want.color, None), (out[3], want.jac, keep)):
        err, tol = _gate(got, w, k)
        print(f"\nquery_source_points colour branch: {err:.3g} / {tol:.3g}")
        assert err <= tol
    # a colour decoder with two hidden levels is not the kernel's: the composed path's result, as before
    dst = cref.random_decoder(8, 32, 3, seed=5, levels=2)
    trk.color_mlp = _ColourDec(dst)
    assert not hnp.colour_fused_supported(trk.neural_points, trk.color_mlp)
    x = cur[:300].cuda()
    got = TO.query_source_points(trk, x, 4096, True, True, True, True, query_locally=True)
    xc = x.clone().requires_grad_(True)
    _, cf, w_knn, _, _ = trk.neural_points.query_feature(xc, accumulate_stability=False, query_locally=True,
                                                         query_color_feature=True, use_only_valid_points=True)
    colc = torch.sum(trk.color_mlp.regress_color(cf) * w_knn, dim=1)
    # the same fp32 operators run twice (the library GEMMs need not be bit-reproducible): a few ulps of a colour in [0, 1]
    assert float((got[2] - colc.detach()).abs().max()) <= 1e-6
    for c in range(3):
        gc = torch.autograd.grad(colc[:, c].sum(), xc, retain_graph=True)[0]
        assert float((got[3][:, c] - gc).abs().max()) <= 1e-5 * float(gc.abs().max())
