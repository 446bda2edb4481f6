"""Device-resident odometry loop (pings_amd.tracker_ops.tracking / registration_step, csrc/tracker.hip
pings_reg_transform / _assemble / _step) against the reference's own runs (tests/golden/tracking_*.npz,
tools/make_tracking_golden.py) and the restatement of the loop (tests/tracking_ref.py)."""
import math
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import tracking_ref as ref

GOLDEN = Path(__file__).parent / "golden"
CASES = ["default", "normals_div_batched", "far"]
TOL_ROT, TOL_T = 1e-4, 1e-4      # rad, m


def _fix(name):
    z = np.load(GOLDEN / f"tracking_{name}.npz")
    return {k: z[k] for k in z.files}


def _cfg(st, **kw):
    c = NS(color_on=False, photometric_loss_on=False, consist_wieght_on=False, weighted_first=bool(st["weighted_first"]),
           color_channel=3, query_nn_k=int(st["nn_k"]))
    for k in st:
        if k.startswith("cfg."):
            v = st[k].item()
            setattr(c, k[4:], v)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _tracker(st, cfg):
    from test_sdf import _Dec, _gpu_map

    return NS(config=cfg, neural_points=_gpu_map(st), sdf_mlp=_Dec(st), silence=True, device="cuda")


def _rot_err(A, B):
    """Angle (rad) of A[:3,:3] B[:3,:3]^T and |A[:3,3] - B[:3,3]|."""
    A, B = torch.as_tensor(A).double().cpu(), torch.as_tensor(B).double().cpu()
    R = A[:3, :3] @ B[:3, :3].T
    c = max(-1.0, min(1.0, (float(torch.trace(R)) - 1.0) / 2.0))
    return math.acos(c), float((A[:3, 3] - B[:3, 3]).norm())


def _room(n, seed, L=(8.0, 6.0, 3.0)):
    """Points on the faces of the fixtures' room (tools/make_tracking_golden.py) with their inward normals."""
    g = torch.Generator().manual_seed(seed)
    Lt = torch.tensor(L)
    areas = torch.tensor([L[1] * L[2], L[1] * L[2], L[0] * L[2], L[0] * L[2], L[0] * L[1], L[0] * L[1]])
    face = torch.multinomial(areas / areas.sum(), n, replacement=True, generator=g)
    p = torch.rand(n, 3, generator=g) * Lt
    nrm = torch.zeros(n, 3)
    for f in range(6):
        m = face == f
        p[m, f // 2] = Lt[f // 2] if f % 2 else 0.0
        nrm[m, f // 2] = -1.0 if f % 2 else 1.0
    return p, nrm


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_runs(name):
    st = _fix(name)
    cfg = _cfg(st)
    npm, dec = ref.cpu_map(st)
    q = ref.cpu_query(npm, dec, int(cfg.infer_bs), int(cfg.track_mask_query_nn_k))
    src = torch.as_tensor(st["src"]).double()
    init = torch.as_tensor(st["init_pose"])
    nrm = torch.as_tensor(st["normals"]).double() if "normals" in st else None
    T, valid, trace = ref.tracking(q, ref.cpu_solve, cfg, src, init, normals=nrm)
    assert len(trace) == int(st["iterations"]) and valid == bool(st["valid_flag"])
    for i, (dT, cnt, res) in enumerate(trace):
        er, et = _rot_err(dT, st["delta"][i])
        assert er <= TOL_ROT and et <= TOL_T, (i, er, et)
        assert abs(cnt - int(st["count"][i])) <= max(2, 1e-3 * cnt), (i, cnt, st["count"][i])
        assert abs(res - float(st["residual"][i])) <= 1e-3 * max(1.0, abs(float(st["residual"][i]))), i
    er, et = _rot_err(T, st["T"])
    assert er <= TOL_ROT and et <= TOL_T
    if bool(st["returned_init"]):
        assert T is init


def test_signatures_are_the_references():
    import inspect

    from pings_amd import tracker_ops as TO

    st = _fix("default")
    s = lambda f: str(inspect.signature(f)).replace("'", "")
    assert s(TO.tracking) == str(st["sig_tracking"])
    assert s(TO.registration_step) == str(st["sig_registration_step"])


def _fake_module():
    calls = []

    class Tracker:
        def tracking(self, *a, **kw):
            calls.append(("tracking", a, kw))
            return "orig-tracking"

        def registration_step(self, *a, **kw):
            calls.append(("registration_step", a, kw))
            return "orig-step"

        def query_source_points(self, *a, **kw):
            raise AssertionError

    return NS(Tracker=Tracker, implicit_reg=None), calls


def test_install_rebinds_what_it_rebinds_and_loop_adds_two_methods():
    from pings_amd import tracker_ops as TO

    m, _ = _fake_module()
    orig_tr, orig_rs = m.Tracker.tracking, m.Tracker.registration_step
    TO.install(m)
    assert m.Tracker.query_source_points is TO.query_source_points and m.implicit_reg is TO.implicit_reg
    assert m.Tracker.tracking is orig_tr and m.Tracker.registration_step is orig_rs
    TO.install(m, loop=True)
    assert m.Tracker.tracking is TO.tracking and m.Tracker.registration_step is TO.registration_step
    assert TO._ORIG["tracking"] is orig_tr and TO._ORIG["registration_step"] is orig_rs
    TO.install(m, loop=True)      # a second install keeps the originals
    assert TO._ORIG["tracking"] is orig_tr


@pytest.mark.parametrize("branch", ["photometric_loss_on", "consist_wieght_on"])
def test_colour_configurations_call_the_saved_original(branch):
    from pings_amd import tracker_ops as TO

    m, calls = _fake_module()
    TO.install(m, loop=True)
    cfg = _cfg(_fix("default"), color_on=True, **{branch: True})
    self = m.Tracker()
    self.config = cfg
    src, col = torch.rand(50, 3), torch.rand(50, 3)
    assert self.tracking(src, None, col) == "orig-tracking"
    assert self.registration_step(src, None, torch.zeros(50), col, 0.4, 2.5) == "orig-step"
    assert [c[0] for c in calls] == ["tracking", "registration_step"]
    assert calls[0][1][0] is src and calls[0][1][2] is col


def test_cpu_tensors_raise():
    from pings_amd import _lib, tracker_ops as TO

    cfg = _cfg(_fix("default"))
    self = NS(config=cfg, silence=True)
    with pytest.raises(_lib.PingsHipError):
        TO.tracking(self, torch.rand(50, 3))
    with pytest.raises(_lib.PingsHipError):
        TO.registration_step(self, torch.rand(50, 3), None, torch.zeros(50), None, 0.4, 2.5)


def test_new_symbols_are_declared_in_the_header():
    import abi_header

    syms = set(abi_header.header_symbols())
    for n in ("transform", "assemble", "step", "partials", "read_record"):
        assert "pings_reg_" + n in syms


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_tracking_matches_the_reference_runs(name):
    from pings_amd import tracker_ops as TO

    st = _fix(name)
    trk = _tracker(st, _cfg(st))
    src = torch.as_tensor(st["src"]).cuda()
    init = torch.as_tensor(st["init_pose"]).cuda()
    nrm = torch.as_tensor(st["normals"]).cuda() if "normals" in st else None
    T, cov, wpc, valid = TO.tracking(trk, src, init, source_normals=nrm)
    tr = TO.last_trace.cpu()
    assert tr.shape[0] == int(st["iterations"]) and valid == bool(st["valid_flag"])
    assert cov is None and wpc is None
    for i in range(tr.shape[0]):
        er, et = _rot_err(tr[i, 8:].view(4, 4), st["delta"][i])
        assert er <= TOL_ROT and et <= TOL_T, (i, er, et)
        assert abs(int(tr[i, 0]) - int(st["count"][i])) <= max(2, 1e-3 * float(tr[i, 0])), i
        assert abs(float(tr[i, 1]) - float(st["residual"][i])) <= 1e-3 * max(1.0, float(st["residual"][i])), i
    if bool(st["returned_init"]):
        assert T is init
    er, et = _rot_err(T, st["T"])
    assert er <= TOL_ROT and et <= TOL_T


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["default", "normals_div_batched"])
def test_hip_registration_step_matches_the_first_iteration(name):
    from pings_amd import tracker_ops as TO

    st = _fix(name)
    cfg = _cfg(st)
    trk = _tracker(st, cfg)
    init = torch.as_tensor(st["init_pose"]).cuda()
    src = torch.as_tensor(st["src"]).cuda()
    cur = ref.transform(src, init)
    nrm = torch.as_tensor(st["normals"]).cuda() if "normals" in st else None
    labels = torch.zeros(src.shape[0], device="cuda")
    GMd = cfg.reg_GM_dist_m if cfg.reg_GM_dist_m > 0 else None
    GMg = cfg.reg_GM_grad if cfg.reg_GM_grad > 0 else None
    out = TO.registration_step(trk, cur, nrm, labels, None, cfg.reg_min_grad_norm, cfg.reg_max_grad_norm, GMd, GMg,
                               cfg.reg_lm_lambda)
    assert len(out) == 7 and out[1] is None and out[2] is None and out[3] is None and out[6] is None
    er, et = _rot_err(out[0], st["delta"][0])
    assert er <= TOL_ROT and et <= TOL_T
    assert isinstance(out[5], float) and abs(out[5] - float(st["residual"][0])) <= 1e-3 * float(st["residual"][0])
    # the valid set is the restatement's over the same HIP query, point for point
    q = _hip_query(trk, cfg)
    _, n, _, valid = ref.step(q, _hip_solve, cfg, cur, nrm, labels, GMd, GMg, cfg.reg_lm_lambda)
    assert torch.equal(out[4], cur[valid]) and n == out[4].shape[0]


def _hip_query(trk, cfg):
    from pings_amd import tracker_ops as TO

    def q(points):
        s, g, _, _, _, m, _, std = TO.query_source_points(trk, points, int(cfg.infer_bs), True, True, False, False,
                                                          query_locally=True,
                                                          mask_min_nn_count=int(cfg.track_mask_query_nn_k))
        return s, g, m, std
    return q


def _hip_solve(points, grad, res, w, lm):
    from pings_amd import tracker_ops as TO

    return TO.implicit_reg(points, grad, res, w, lm)[0]


GRID = [dict(reg_GM_dist_m=0.3, reg_GM_grad=0.1, reg_lm_lambda=1e-4, normals=False, infer_bs=32768),
        dict(reg_GM_dist_m=0.0, reg_GM_grad=0.0, reg_lm_lambda=0.0, normals=False, infer_bs=32768),
        dict(reg_GM_dist_m=0.3, reg_GM_grad=0.0, reg_lm_lambda=1e-4, normals=True, infer_bs=6000),
        dict(reg_GM_dist_m=0.0, reg_GM_grad=0.1, reg_lm_lambda=0.0, normals=True, infer_bs=4096,
             reg_dist_div_grad_norm=True)]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(GRID)))
def test_hip_tracking_matches_the_restatement_on_a_20k_scan(k):
    """The loop against the restatement driven by today's HIP drop-ins (query_source_points, implicit_reg) over GM
    on / off, normals on / off, LM 0 / 1e-4 and batched queries, on a 20k-point scan of the fixtures' room."""
    from pings_amd import tracker_ops as TO

    st = _fix("default")
    opt = dict(GRID[k])
    use_n = opt.pop("normals")
    cfg = _cfg(st, **opt)
    trk = _tracker(st, cfg)
    T_gt = torch.as_tensor(st["T_gt"])
    w, nw = _room(20000, seed=100 + k)
    Ti = torch.linalg.inv(T_gt)
    src = (w.double() @ Ti[:3, :3].T + Ti[:3, 3]).float().cuda()
    nrm = (nw.double() @ Ti[:3, :3].T).float().cuda() if use_n else None
    init = torch.as_tensor(st["init_pose"]).cuda()
    T, valid, trace = ref.tracking(_hip_query(trk, cfg), _hip_solve, cfg, src, init.clone(), normals=nrm)
    Td, _, _, valid_d = TO.tracking(trk, src, init.clone(), source_normals=nrm)
    tr = TO.last_trace.cpu()
    assert tr.shape[0] == len(trace) and valid_d == valid
    for i, (dT, cnt, res) in enumerate(trace):
        er, et = _rot_err(tr[i, 8:].view(4, 4), dT)
        assert er <= TOL_ROT and et <= TOL_T, (i, er, et)
        assert abs(int(tr[i, 0]) - cnt) <= 2 and abs(float(tr[i, 1]) - res) <= 1e-3 * max(1.0, res), i
    er, et = _rot_err(Td, T)
    assert er <= TOL_ROT and et <= TOL_T


@pytest.mark.gpu
def test_hip_tracking_reads_the_host_once_per_iteration_and_is_deterministic():
    from pings_amd import _lib, tracker_ops as TO

    st = _fix("normals_div_batched")
    trk = _tracker(st, _cfg(st))
    src = torch.as_tensor(st["src"]).cuda()
    init = torch.as_tensor(st["init_pose"]).cuda()
    nrm = torch.as_tensor(st["normals"]).cuda()
    TO.tracking(trk, src, init, source_normals=nrm)     # warm-up: first-use allocations and reads of the map
    torch.cuda.synchronize()
    _lib.sync_counts(reset=True)
    torch.cuda.set_sync_debug_mode("error")
    try:
        T1, _, _, v1 = TO.tracking(trk, src, init, source_normals=nrm)
        tr1 = TO.last_trace
    finally:
        torch.cuda.set_sync_debug_mode(0)
    counts = _lib.sync_counts(reset=True)
    assert counts == {"tracking_iteration": tr1.shape[0]}
    T2, _, _, v2 = TO.tracking(trk, src, init, source_normals=nrm)
    assert torch.equal(T1, T2) and v1 == v2 and torch.equal(tr1, TO.last_trace)


@pytest.mark.gpu
def test_hip_tracking_raises_on_a_singular_system(monkeypatch):
    """A plane z = 0 seen with the exact gradient (0, 0, 1): rotation about z and translation in x, y are not
    observed, their rows of N are exactly zero; the reference's torch.linalg.inv raises LinAlgError."""
    from pings_amd import tracker_ops as TO

    n = 500
    g = torch.Generator().manual_seed(1)
    src = torch.cat([torch.rand(n, 2, generator=g) * 4, torch.zeros(n, 1)], 1).cuda()

    def flat(self, coord, bs, *a, **kw):
        m = coord.shape[0]
        grad = torch.zeros(m, 3, device=coord.device)
        grad[:, 2] = 1.0
        return (torch.full((m,), 0.01, device=coord.device), grad, None, None, None,
                torch.ones(m, dtype=torch.bool, device=coord.device), None, torch.zeros(m, device=coord.device))

    monkeypatch.setattr(TO, "query_source_points", flat)
    st = _fix("default")
    trk = NS(config=_cfg(st), silence=True)
    with pytest.raises(torch.linalg.LinAlgError):
        TO.tracking(trk, src)


@pytest.mark.gpu
def test_hip_vis_iteration_gives_the_reference_path_the_device_pose():
    from pings_amd import tracker_ops as TO

    st = _fix("default")
    seen = {}

    class Tracker:
        def registration_step(self, points, *a, **kw):
            seen["points"] = points.clone()
            seen["vis"] = a[-1]
            return (torch.eye(4, dtype=torch.float64, device=points.device), None, None, "cloud", points[:2900],
                    1.0, None)

    m = NS(Tracker=Tracker, implicit_reg=None)
    TO.install(m, loop=True)
    try:
        trk = _tracker(st, _cfg(st))
        src = torch.as_tensor(st["src"]).cuda()
        init = torch.as_tensor(st["init_pose"]).cuda()
        T, cov, wpc, valid = TO.tracking(trk, src, init, vis_result=True)
    finally:
        TO._ORIG.clear()
    assert wpc == "cloud" and seen["vis"] is True and valid
    tr = TO.last_trace.cpu()
    pose = torch.as_tensor(st["init_pose"])
    for i in range(tr.shape[0] - 1):
        pose = tr[i, 8:].view(4, 4) @ pose
    assert torch.allclose(pose, T.cpu().double(), atol=1e-12)     # the delegated step was the identity
    assert (seen["points"].cpu() - ref.transform(src.cpu(), pose)).abs().max() <= 1e-5
