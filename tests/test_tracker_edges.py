"""The tracker's step kernels (pings_amd/csrc/tracker.hip) through the C ABI, with chosen inputs, against the fp64
restatement of tests/tracker_edges_ref.py: every size at which a grid-stride loop takes another pass, rows that sit
exactly on the validity window, the 9 / 10 valid-point early return, the record and trace layout, and the 6x6 solve on
hand-made systems (row swap, conditioning threshold, tiny and near-pi angles, fp32 damping).

Bounds.  u = 2^-24 is the unit roundoff of fp32.  One term w J_a J_b of the normal equations carries at most 16 fp32
roundings in the kernel (12 in the chain |g| -> residual -> weights, 3 in a cross-product entry whether or not the
multiply-add is fused, 1 spare), each relative to the magnitudes of that step, so a sum over points is within
16 u S_ab of the fp64 sum, S_ab being the sum of the terms' magnitudes with |p_y g_z| + |p_z g_y| in place of the
cross-product entry.  The kernel accumulates in fp64: below n 2^-52 relative, added to the bound.  The CPU tests at
the top check, without a device, that the reference's own fp32 arithmetic stays within a quarter of each bound on the
very inputs the device tests use, and that fp32 and fp64 decide every point's validity alike.
"""
import ctypes as C
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import tracker_edges_ref as R
import tracking_ref

U = 2.0 ** -24
EPS = 2.0 ** -52
ASSEMBLE_ROUNDINGS = 16      # 12 residual / weight chain + 3 cross product + 1 spare
NORMAL_EQ_ROUNDINGS = 4      # 3 cross product + 1 output
TRANSFORM_ROUNDINGS = 4      # a product and the three additions behind it
STEP_N = 300                 # two workgroups, the second partly filled

TRANSFORM_SIZES = (1, 255, 257, 524288, 524289)


def _seed(n, name):
    return 1000 + 13 * n + sorted(R.FLAG_SETS).index(name)


@functools.lru_cache(maxsize=None)
def _case(n, flagset, label_nonzero=False, offset=1000.0):
    """(inputs, settings, fp64 restatement) of one assemble case; shared by the CPU and the device tests, never modified."""
    inp = R.make_inputs(n, _seed(n, flagset), offset=offset, label_nonzero=label_nonzero, all_valid=n < 64)
    st = R.settings(flagset)
    return inp, st, R.assemble(inp, st)


@functools.lru_cache(maxsize=None)
def _step_case(flagset, keep=None):
    """Inputs of the step tests: the same rows in a box around the origin, where rotation and translation separate
    (around an offset of 1000 m the 2-norm condition number of N is ~1e11)."""
    inp = R.make_inputs(STEP_N, _seed(STEP_N, flagset) + 5, offset=0.0, label_nonzero=True)
    st = R.settings(flagset)
    if keep is not None:
        inp = R.limit_valid(inp, R.assemble(inp, st).valid.numpy(), keep)
    return inp, st, R.assemble(inp, st)


@functools.lru_cache(maxsize=None)
def _normal_eq_case(n):
    p, g, r, w = R.make_normal_eq_inputs(n, 77 + n)
    return (p, g, r, w), R.normal_equations(p, g, r, w)


def _pose():
    """A pose with a rotation (0.7 rad about a skew axis) and a translation of 1000 m."""
    T = np.eye(4)
    T[:3, :3] = R.expmap(0.7 * np.array([0.6, -0.48, 0.64]))
    T[:3, 3] = (1000.0, -730.0, 12.5)
    return T


def _ratio(err, bound):
    """max err / bound over the entries; an entry whose bound is 0 must be exact."""
    err, bound = np.asarray(err, np.float64).ravel(), np.asarray(bound, np.float64).ravel()
    assert np.all(err[bound == 0] == 0), "an entry without any contribution is not exactly zero"
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ================================================================ CPU: the helper and the bounds
def test_edge_rows_are_decided_as_written_in_both_precisions():
    inp, st, ref = _case(257, "all")
    assert inp.edge.sum() == 2 * R.edge_rows()[0].shape[0] and inp.edge[-1] and inp.edge[0]
    for dtype in (torch.float64, torch.float32):
        valid = R.assemble(inp, st, dtype).valid.numpy()
        assert np.array_equal(valid[inp.edge], inp.edge_valid[inp.edge])
    assert inp.edge_valid.sum() == 2 * 3      # the three inner neighbours, twice


@pytest.mark.parametrize("flagset", sorted(R.FLAG_SETS))
def test_helper_agrees_with_the_loop_restatement(flagset):
    """tests/tracking_ref.py:step with oracle/tracker_cpu.implicit_reg, all in float64 and driven by a query that returns
    the prepared arrays, against `assemble` + `step`: same mask and count, residual mean to 1e-12, dT within the
    conditioning of the fp64 solve (torch.linalg.inv @ g against numpy.linalg.solve: both within c cond_2 2^-53 of the
    exact solution, tracker_edges_ref.solve_tolerance; tests/test_tracker.py sets its 1e-7 for an N of cond ~1e6 so)."""
    inp, st, ref = _step_case(flagset)
    d = lambda a: torch.as_tensor(a).double()
    cfg = NS(surface_sample_range_m=st["max_std"], max_sdf_std_ratio=1.0, reg_max_grad_norm=st["max_grad"],
             reg_min_grad_norm=st["min_grad"], reg_dist_div_grad_norm=bool(st["flags"] & R.F_DIV_GRAD))
    query = lambda pts: (d(inp.sdf), d(inp.grad), torch.as_tensor(inp.mask).bool(), d(inp.std))
    dT, n, res_cm, valid = tracking_ref.step(query, tracking_ref.cpu_solve, cfg, d(inp.cur),
                                             d(inp.normals) if st["flags"] & R.F_NORMALS else None, d(inp.label),
                                             st["gm_dist"] or None, st["gm_grad"] or None, st["lm_lambda"])
    assert torch.equal(valid, ref.valid) and n == ref.count and n >= 50
    assert abs(res_cm - ref.sum_abs_r / ref.count * 100.0) <= 1e-12
    weighted = bool(st["flags"] & R.F_WEIGHTED)
    c = ref.count / (2.0 * ref.sum_w) if weighted else 1.0
    ng = np.concatenate([c * ref.N.numpy().reshape(36), c * ref.g.numpy()])     # fp64: damped in fp64, as the oracle
    s = R.step(ng, st["lm_lambda"])
    assert s.cond <= 1e6
    err = np.abs(dT.numpy() - s.dT).max()
    print(f"\n[{flagset}] cond {s.cond:.3g}  |dT - dT_ref| {err:.3g}  allowed {R.solve_tolerance(s.cond) * np.abs(s.t).max():.3g}")
    assert err <= R.solve_tolerance(s.cond) * np.abs(s.t).max() + 16 * EPS


@pytest.mark.parametrize("n,flagset,label_nonzero", R.ASSEMBLE_CASES)
def test_fp32_restatement_is_within_a_quarter_of_the_assemble_bound(n, flagset, label_nonzero):
    inp, st, ref = _case(n, flagset, label_nonzero)
    f32 = R.assemble(inp, st, torch.float32)
    assert torch.equal(f32.valid, ref.valid) and f32.count == ref.count       # no undecidable point
    assert ref.count == n if n < 64 else 0.2 * n < ref.count < 0.7 * n
    ratio = _ratio(np.abs(R.totals(f32) - R.totals(ref)), ASSEMBLE_ROUNDINGS * U * R.total_bounds(ref))
    print(f"\n[n={n} {flagset}] valid {ref.count}  fp32 restatement error / bound {ratio:.3f}")
    assert ratio <= 0.25


@pytest.mark.parametrize("flagset,keep", [(fs, None) for fs in sorted(R.FLAG_SETS)] + [("all", 9), ("all", 10)])
def test_step_inputs_are_well_conditioned_and_inside_the_bound(flagset, keep):
    inp, st, ref = _step_case(flagset, keep)
    f32 = R.assemble(inp, st, torch.float32)
    assert torch.equal(f32.valid, ref.valid) and (keep is None or ref.count == keep)
    assert _ratio(np.abs(R.totals(f32) - R.totals(ref)), ASSEMBLE_ROUNDINGS * U * R.total_bounds(ref)) <= 0.25
    if ref.count >= 10:
        for weighted in (False, True):
            assert R.step(R.normal_eq_from_totals(R.totals(f32), weighted), st["lm_lambda"]).cond <= 1e6


@pytest.mark.parametrize("n", R.NORMAL_EQ_SIZES)
def test_fp32_restatement_is_within_a_quarter_of_the_normal_equation_bound(n):
    (p, g, r, w), ref = _normal_eq_case(n)
    f32 = R.normal_equations(p, g, r, w, torch.float32)
    got = np.concatenate([f32.N.numpy().ravel(), f32.g.numpy()]).astype(np.float32).astype(np.float64)
    want = np.concatenate([ref.N.numpy().ravel(), ref.g.numpy()])
    bound = NORMAL_EQ_ROUNDINGS * U * np.concatenate([ref.S.numpy().ravel(), ref.Sg.numpy()])
    ratio = _ratio(np.abs(got - want), bound + np.where(bound > 0, np.spacing(np.abs(want).astype(np.float32)), 0))
    print(f"\n[n={n}] fp32 restatement error / bound {ratio:.3f}")
    assert ratio <= 0.25


def test_fp32_transform_is_within_its_bound():
    """The worst of 1.5 million coordinates comes close to what four roundings can do: the bound itself is asserted."""
    src, M, want, bound = _transform_case(524289)
    got = ((M[:3, 0] * src[:, :1] + M[:3, 1] * src[:, 1:2]) + M[:3, 2] * src[:, 2:3]) + M[:3, 3]
    ratio = _ratio(np.abs(got.astype(np.float64) - want), bound)
    print(f"\nfp32 transform error / bound {ratio:.3f}")
    assert got.dtype == np.float32 and ratio <= 1.0


# ---------------------------------------------------------------- hand-made systems of the solve tests
def _spd(cond, seed):
    """Symmetric positive definite 6x6 with eigenvalues from 1 down to 1 / cond, rounded to fp32 (symmetric still)."""
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(6, 6)))
    A = (q * np.logspace(0.0, -np.log10(cond), 6)) @ q.T
    return ((A + A.T) / 2).astype(np.float32)


def _swapped(zero=False):
    """Symmetric, leading diagonal entry 1e-6 of the rest (or exactly 0): the first pivot is another row."""
    A = _spd(10.0, 5).copy()
    A[0, 0] = 0.0 if zero else 1e-6 * A[1, 1]
    assert np.abs(A[1:, 0]).max() > 1e3 * abs(A[0, 0])
    return A


ANGLES = {"tiny": 1e-9, "one": 1.0, "near_pi": np.pi - 5e-7}
SYSTEMS = {"cond10": lambda: _spd(10.0, 1), "cond1e3": lambda: _spd(1e3, 2), "swap": _swapped,
           "swap_zero": lambda: _swapped(True)}


@functools.lru_cache(maxsize=None)
def _system(name, lam, angle):
    """[N | g] in fp32 whose step has a rotation angle within 1e-6 (relative 1e-6 for the tiny one) of ANGLES[angle]."""
    N, target = SYSTEMS[name](), ANGLES[angle]
    g = np.random.default_rng(9).normal(size=6)
    for _ in range(50):
        ng = np.concatenate([N.ravel(), g]).astype(np.float32)
        a = np.linalg.norm(R.step(ng, lam).t[:3])
        if abs(a - target) <= 2e-7 * min(target, 1.0):
            break
        g = ng[36:].astype(np.float64) * (target / a)
    s = R.step(ng, lam)
    assert abs(np.linalg.norm(s.t[:3]) - target) <= 1e-6 * min(target, 1.0)
    return ng, s


def _min_pivot_ratio(A):
    """Smallest |pivot| of Gaussian elimination with partial pivoting over the largest |entry| (the kernel's measure)."""
    A = A.copy()
    scale, piv = np.abs(A).max(), []
    for k in range(6):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, p]] = A[[p, k]]
        piv.append(abs(A[k, k]))
        A[k + 1:] -= np.outer(A[k + 1:, k] / A[k, k], A[k])
    return min(piv) / scale


SOLVE_CASES = [(m, lam, a) for m in ("cond10", "cond1e3") for lam in (0.0, R.f32(1e-4), 0.5) for a in ANGLES] + \
              [(m, 0.0, a) for m in ("swap", "swap_zero") for a in ANGLES]


def test_solve_systems_are_what_they_are_called():
    for name, lo, hi in (("cond10", 9.0, 11.0), ("cond1e3", 900.0, 1100.0)):
        assert lo <= np.linalg.cond(SYSTEMS[name]().astype(np.float64), 2) <= hi
    for name in ("swap", "swap_zero"):
        A = SYSTEMS[name]().astype(np.float64)
        assert np.array_equal(A, A.T) and np.argmax(np.abs(A[:, 0])) != 0 and np.linalg.cond(A, 2) <= 1e3
    for m, lam, a in SOLVE_CASES:
        ng, s = _system(m, lam, a)
        assert _min_pivot_ratio(R.damped(ng, lam)) >= 1e-5       # status 0 expected: far above the kernel's 1e-7
    assert abs(np.linalg.norm(_system("cond10", 0.0, "near_pi")[1].t[:3]) - np.pi) <= 1e-6


def _transform_case(n):
    rng = np.random.default_rng(n)
    src = rng.uniform(-40.0, 40.0, (n, 3)).astype(np.float32)
    M = _pose().astype(np.float32)                                   # T.to(fp32), as the kernel casts it
    s64, M64 = src.astype(np.float64), M.astype(np.float64)
    want = s64 @ M64[:3, :3].T + M64[:3, 3]
    bound = TRANSFORM_ROUNDINGS * U * (np.abs(s64) @ np.abs(M64[:3, :3]).T + np.abs(M64[:3, 3]))
    return src, M, want, bound


# ================================================================ device
def _lib():
    from pings_amd import _lib as L

    return L, L.lib()


def _up(a, rows):
    """The array on the device in a buffer of at least one row: no kernel is ever handed a null or short buffer."""
    a = np.ascontiguousarray(a)
    t = torch.zeros((max(rows, 1),) + a.shape[1:], dtype=torch.from_numpy(a[:0].copy()).dtype, device="cuda")
    t[:a.shape[0]] = torch.from_numpy(a)
    return t


class _Dev:
    """Buffers and argument block of the loop kernels, allocated at full size as pings_amd.tracker_ops._Loop does."""

    def __init__(self, inp, st, pose=None, trace_rows=0, trace_cap=None, src=None):
        from pings_amd import _abi

        self.mod, self.L = _lib()
        n = self.n = int(inp.n)
        self.buf = {k: _up(getattr(inp, k), n) for k in ("cur", "sdf", "grad", "std", "mask", "label", "normals")}
        self.src = _up(inp.cur if src is None else src, n)
        self.nb = int(self.L.pings_reg_partials(n))
        assert self.nb == min(max((n + 255) // 256, 1), 256)
        self.part = torch.full((self.nb * 32,), -7.0, dtype=torch.float64, device="cuda")
        self.T = torch.from_numpy(np.eye(4) if pose is None else pose.copy()).cuda()
        self.delta = torch.full((4, 4), -7.0, dtype=torch.float64, device="cuda")
        self.record = torch.full((8,), -7, dtype=torch.int32, device="cuda")
        self.valid = torch.full((max(n, 1),), 7, dtype=torch.uint8, device="cuda")
        self.trace = torch.full((trace_rows, 24), -12345.678, dtype=torch.float64, device="cuda") if trace_rows else None
        a = _abi.RegLoopArgs(n, st["flags"], 0, trace_rows if trace_cap is None else trace_cap, st["min_grad"],
                             st["max_grad"], st["max_std"], st["gm_dist"], st["gm_grad"], st["lm_lambda"])
        a.src, a.cur, a.sdf, a.grad, a.std = (t.data_ptr() for t in (self.src, self.buf["cur"], self.buf["sdf"],
                                                                     self.buf["grad"], self.buf["std"]))
        a.mask, a.label = self.buf["mask"].data_ptr(), self.buf["label"].data_ptr()
        a.normals = self.buf["normals"].data_ptr() if st["flags"] & R.F_NORMALS else None
        a.valid = self.valid.data_ptr()
        a.part, a.T, a.delta, a.record = (t.data_ptr() for t in (self.part, self.T, self.delta, self.record))
        a.trace = self.trace.data_ptr() if trace_rows else None
        self.a = a
        self.stream = self.mod.stream_ptr(torch.device("cuda", torch.cuda.current_device()))

    def call(self, name):
        rc = getattr(self.L, "pings_reg_" + name)(C.byref(self.a), self.stream)
        assert rc == 0, (name, self.L.pings_last_error())

    def partials(self):
        return self.part.cpu().numpy().reshape(self.nb, 32)

    def totals(self):
        """The per-block sums added in block order in fp64: what the step kernel adds, bit for bit."""
        tot = np.zeros(32)
        for row in self.partials():
            tot = tot + row
        return tot

    def host_record(self):
        host = (C.c_int32 * 8)()
        assert self.L.pings_reg_read_record(self.record.data_ptr(), C.addressof(host), self.stream) == 0
        rec = np.frombuffer(bytes(host), np.int32)
        assert np.array_equal(rec, self.record.cpu().numpy())
        return int(rec[0]), int(rec[1]), rec[2:].copy().view(np.float64)


def _check_assemble(dev, inp, ref, tag):
    got_valid = dev.valid.cpu().numpy()[:inp.n].astype(bool)
    assert np.array_equal(got_valid, ref.valid.numpy()), np.flatnonzero(got_valid != ref.valid.numpy())[:10]
    tot = dev.totals()
    assert tot[27] == ref.count and tot[31] == 0.0
    per_term = ASSEMBLE_ROUNDINGS * U + inp.n * EPS
    ratio = _ratio(np.abs(tot - R.totals(ref)), per_term * R.total_bounds(ref))
    print(f"\n[{tag}] valid {ref.count}  error / bound {ratio:.3f}")
    assert ratio <= 1.0
    return tot


@pytest.mark.gpu
@pytest.mark.parametrize("n,flagset,label_nonzero", R.ASSEMBLE_CASES)
def test_assemble_matches_fp64(n, flagset, label_nonzero):
    """valid[n] exactly, the count exactly, every sum within 16 u of its magnitude sum (module docstring); two launches
    bit-equal; valid == NULL accepted and without effect on the sums.  n = 65,537 is the first size at which the 256
    workgroups of 256 take a second grid-stride pass, at 131,073 one thread takes a third."""
    inp, st, ref = _case(n, flagset, label_nonzero)
    dev = _Dev(inp, st)
    dev.call("assemble")
    _check_assemble(dev, inp, ref, f"assemble n={n} {flagset}")
    first = dev.partials()
    dev.part.fill_(-7.0)
    dev.call("assemble")
    assert np.array_equal(_bits(first), _bits(dev.partials()))
    dev.part.fill_(-7.0)
    dev.valid.fill_(7)
    dev.a.valid = None
    dev.call("assemble")
    assert np.array_equal(_bits(first), _bits(dev.partials()))
    assert bool((dev.valid == 7).all())


def _check_step(dev, st, pose, it=0):
    """The step against the helper fed the kernel's own fp32 [N | g] (from the partials): solve and pose update only."""
    tot = dev.totals()
    ng = R.normal_eq_from_totals(tot, bool(dev.a.flags & R.F_WEIGHTED))
    ref = R.step(ng, st["lm_lambda"], pose)
    assert ref.cond <= 1e6
    tol, tn = R.solve_tolerance(ref.cond), np.abs(ref.t).max()
    delta, T = dev.delta.cpu().numpy(), dev.T.cpu().numpy()
    # |d delta| <= tol |t|_inf (solve; the exponential map has unit gain) + a few ulps of sin / cos; T = delta @ pose
    bd = np.full((4, 4), tol * tn + 16 * EPS)
    bd[3] = 0.0
    r1 = _ratio(np.abs(delta - ref.dT), bd)
    r2 = _ratio(np.abs(T - ref.T), bd @ np.abs(pose) + 16 * EPS * (np.abs(ref.dT) @ np.abs(pose)))
    cnt, status, vals = dev.host_record()
    assert cnt == int(tot[27]) and status == 0
    assert vals[0] == float(np.float32(tot[29] / tot[27])) * 100.0               # torch.mean of fp32 |r|, .item(), * 100
    assert abs(vals[1] - R.rot_deg(ref.dT)) <= 1e-9 and abs(vals[2] - R.tran_m(ref.dT)) <= 1e-9
    assert vals[1] > 1e-3 and vals[2] > 1e-4, "not a real step"
    if dev.trace is not None:
        row = dev.trace.cpu().numpy()[it]
        assert np.array_equal(_bits(row[1:4]), _bits(vals))
        assert row[0] == cnt and row[4] == status and row[5] == tot[28] and row[6] == tot[30] and row[7] == 0.0
        assert np.array_equal(_bits(row[8:]), _bits(delta.ravel()))
    print(f"  cond {ref.cond:.3g}  delta error / bound {r1:.3g}  T error / bound {r2:.3g}")
    assert r1 <= 1.0 and r2 <= 1.0
    return delta


@pytest.mark.gpu
@pytest.mark.parametrize("flagset", sorted(R.FLAG_SETS))
def test_step_matches_the_fp64_solve_of_the_kernels_own_system(flagset):
    inp, st, ref = _step_case(flagset)
    pose = _pose()
    dev = _Dev(inp, st, pose, trace_rows=2)
    dev.a.iter = 1
    dev.call("assemble")
    _check_assemble(dev, inp, ref, f"step n={inp.n} {flagset}")
    dev.call("step")
    _check_step(dev, st, pose, it=1)
    assert bool((dev.trace[0] == -12345.678).all())


@pytest.mark.gpu
def test_step_returns_early_below_ten_valid_points():
    """registration_step's `if valid_point_count < 10`: with 9 valid points the identity step, the pose untouched bit for
    bit, the record (9, 0, 0.0, 0.0, 0.0); with 10 a real step."""
    pose = _pose()
    for keep in (9, 10):
        inp, st, ref = _step_case("all", keep)
        assert ref.count == keep
        dev = _Dev(inp, st, pose)
        dev.call("assemble")
        _check_assemble(dev, inp, ref, f"step keep={keep}")
        dev.call("step")
        if keep == 9:
            assert np.array_equal(_bits(dev.delta.cpu().numpy()), _bits(np.eye(4)))
            assert np.array_equal(_bits(dev.T.cpu().numpy()), _bits(pose))
            cnt, status, vals = dev.host_record()
            assert (cnt, status) == (9, 0) and np.array_equal(_bits(vals), np.zeros(3, np.int64))
        else:
            _check_step(dev, st, pose)


@pytest.mark.gpu
def test_weighted_flag_rescales_the_system_without_changing_the_step():
    """`w /= 2 mean(w)` multiplies N and g by one factor c = count / (2 sum w), which cancels in N^-1 g.  With unit weights
    c is exactly 1/2: the fp32 rounding of c N, the damping and every elimination step scale exactly, so the two steps
    agree within the conditioning bound of one solve.  With any other c the fp32 rounding of c N differs from that of N
    entry by entry (relative 2^-24 each, in the reference as well), which moves the solution by up to
    2 cond_2 2^-24 |t| per system: that case is held to 4 cond_2 2^-24 + the solve's bound."""
    pose = _pose()
    for flagset, refit in (("none", 0.0), ("all", 4.0 * U)):
        inp, st, ref = _step_case(flagset)
        out = {}
        for weighted in (False, True):
            dev = _Dev(inp, st, pose)
            dev.a.flags = (st["flags"] & ~R.F_WEIGHTED) | (R.F_WEIGHTED if weighted else 0)
            dev.call("assemble")
            dev.call("step")
            s = R.step(R.normal_eq_from_totals(dev.totals(), weighted), st["lm_lambda"])
            out[weighted] = dev.delta.cpu().numpy()
            assert dev.host_record()[1] == 0
        if flagset == "none":
            tot = dev.totals()
            assert tot[27] / (2.0 * tot[28]) == 0.5
        bound = (R.solve_tolerance(s.cond) + refit * s.cond) * np.abs(s.t).max() + 16 * EPS
        err = np.abs(out[True] - out[False]).max()
        print(f"\n[weighted on/off, {flagset}] cond {s.cond:.3g}  |delta_on - delta_off| / bound {err / bound:.3g}")
        assert err <= bound


@pytest.mark.gpu
def test_trace_rows_outside_the_capacity_are_left_alone():
    inp, st, ref = _step_case("all")
    dev = _Dev(inp, st, _pose(), trace_rows=5, trace_cap=3)
    dev.call("assemble")
    sentinel = dev.trace.cpu().numpy().copy()
    for it in (-1, 0, 2, 3):
        dev.a.iter = it
        dev.call("step")
    tr = dev.trace.cpu().numpy()
    same = [np.array_equal(_bits(tr[r]), _bits(sentinel[r])) for r in range(5)]
    assert same == [False, True, False, True, True]
    assert tr[0, 0] == ref.count and tr[2, 0] == ref.count and tr[0, 7] == 0.0


@pytest.mark.gpu
def test_no_points_is_an_identity_step():
    inp, st, _ = _case(0, "all")
    pose = _pose()
    dev = _Dev(inp, st, pose)
    dev.buf["cur"].fill_(3.25)
    for name in ("transform", "assemble", "step"):
        dev.call(name)
    assert bool((dev.buf["cur"] == 3.25).all())
    assert np.array_equal(dev.partials(), np.zeros((1, 32)))
    assert np.array_equal(_bits(dev.delta.cpu().numpy()), _bits(np.eye(4)))
    assert np.array_equal(_bits(dev.T.cpu().numpy()), _bits(pose))
    cnt, status, vals = dev.host_record()
    assert (cnt, status) == (0, 0) and np.array_equal(_bits(vals), np.zeros(3, np.int64))


@pytest.mark.gpu
def test_a_nan_sdf_is_reported_not_raised():
    from pings_amd import _abi

    inp, st, ref = _step_case("all")
    inp = NS(**vars(inp))
    inp.sdf = inp.sdf.copy()
    inp.sdf[np.flatnonzero(ref.valid.numpy())[3]] = np.nan
    dev = _Dev(inp, st, _pose())
    dev.call("assemble")
    dev.call("step")            # returns PINGS_OK
    cnt, status, vals = dev.host_record()
    assert cnt == ref.count and status & _abi.REG_NONFINITE
    assert np.array_equal(dev.valid.cpu().numpy()[:inp.n].astype(bool), ref.valid.numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("n", TRANSFORM_SIZES)
def test_transform_matches_fp64(n):
    """cur = R p + t in fp32 from the pose cast to fp32 (transform_torch): per coordinate within 4 u (|R_r| . |p| + |t_r|),
    the first product passing one multiplication and three additions.  524,289 is the first size at which the 2,048
    workgroups take a second pass."""
    src, M, want, bound = _transform_case(n)
    inp, st, _ = _case(0, "all")
    inp = NS(**{**vars(inp), "n": n, "cur": np.zeros((n, 3), np.float32)})
    for k in ("sdf", "std", "mask", "label"):
        setattr(inp, k, np.zeros(1, getattr(inp, k).dtype))
    inp.grad = inp.normals = np.zeros((1, 3), np.float32)
    pose = _pose()
    dev = _Dev(inp, st, pose, src=src)
    dev.buf["cur"] = torch.full((n + 1, 3), -5.0, device="cuda")       # one guard row behind the output
    dev.a.cur = dev.buf["cur"].data_ptr()
    dev.call("transform")
    out = dev.buf["cur"].cpu().numpy()
    assert np.all(out[n] == -5.0)
    ratio = _ratio(np.abs(out[:n].astype(np.float64) - want), bound)
    print(f"\n[transform n={n}] error / bound {ratio:.3f}")
    assert ratio <= 1.0
    assert np.array_equal(_bits(dev.T.cpu().numpy()), _bits(pose))


@pytest.mark.gpu
@pytest.mark.parametrize("n", R.NORMAL_EQ_SIZES)
def test_normal_equations_match_fp64(n):
    """`pings_reg_normal_equations` (w and r given): within 4 u S_ab (3 roundings of a cross-product entry, 1 of the fp32
    output) plus one ulp of the output; n = 0 gives 42 exact zeros; two calls bit-equal.  131,073 is the first size at
    which the 512 workgroups take a second pass, 262,145 the first with a third."""
    mod, L = _lib()
    (p, g, r, w), ref = _normal_eq_case(n)
    bufs = [_up(a, n) for a in (p, g, r, w)]
    scratch = torch.empty(L.pings_reg_normal_equations_scratch_bytes(), dtype=torch.uint8, device="cuda")
    stream = mod.stream_ptr(torch.device("cuda", torch.cuda.current_device()))
    outs = []
    for _ in range(2):
        out = torch.full((42,), -7.0, device="cuda")
        scratch.fill_(0xFF)
        assert L.pings_reg_normal_equations(*(b.data_ptr() for b in bufs), n, scratch.data_ptr(), out.data_ptr(),
                                            stream) == 0
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0].view(np.int32), outs[1].view(np.int32))
    got = outs[0].astype(np.float64)
    assert np.array_equal(got[:36].reshape(6, 6), got[:36].reshape(6, 6).T)
    if n == 0:
        assert np.array_equal(outs[0].view(np.int32), np.zeros(42, np.int32))
    want = np.concatenate([ref.N.numpy().ravel(), ref.g.numpy()])
    bound = (NORMAL_EQ_ROUNDINGS * U + n * EPS) * np.concatenate([ref.S.numpy().ravel(), ref.Sg.numpy()])
    ratio = _ratio(np.abs(got - want), bound + np.where(bound > 0, np.spacing(np.abs(want).astype(np.float32)), 0))
    print(f"\n[normal equations n={n}] error / bound {ratio:.3f}")
    assert ratio <= 1.0


def _solve(ng, lam):
    mod, L = _lib()
    dev_ng = torch.from_numpy(np.ascontiguousarray(ng, np.float32)).cuda()
    T = torch.full((16,), -7.0, dtype=torch.float64, device="cuda")
    t = torch.full((6,), -7.0, dtype=torch.float64, device="cuda")
    status = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    host = C.c_int32(-7)
    stream = mod.stream_ptr(torch.device("cuda", torch.cuda.current_device()))
    assert L.pings_reg_solve_checked(dev_ng.data_ptr(), float(lam), T.data_ptr(), t.data_ptr(), status.data_ptr(),
                                     C.byref(host), stream) == 0
    assert int(status.item()) == host.value
    return T.cpu().numpy().reshape(4, 4), t.cpu().numpy(), host.value


@pytest.mark.gpu
@pytest.mark.parametrize("name,lam,angle", SOLVE_CASES)
def test_solve_matches_numpy(name, lam, angle):
    """`pings_reg_solve_checked` on hand-made systems against numpy.linalg.solve of the fp32-damped matrix and fp64
    Rodrigues: t within 1e3 cond_2 2^-52 |t|_inf, the pose within that plus a few ulps of sin / cos of each entry's
    own scale (1 on the diagonal, the angle beside it), R orthonormal with det 1 to 1e-12, status 0."""
    ng, ref = _system(name, lam, angle)
    T, t, status = _solve(ng, lam)
    tol, tn = R.solve_tolerance(ref.cond), np.abs(ref.t).max()
    r_t = _ratio(np.abs(t - ref.t), np.full(6, tol * tn))
    ang = min(1.0, float(np.linalg.norm(ref.t[:3])))
    bd = np.full((4, 4), tol * tn)
    bd[:3, :3] += 16 * EPS * (np.eye(3) + ang * (1 - np.eye(3)))
    bd[3] = 0.0
    r_T = _ratio(np.abs(T - ref.dT), bd)
    print(f"\n[solve {name} lambda={lam:g} {angle}] cond {ref.cond:.3g}  t error / bound {r_t:.3g}  T error / bound {r_T:.3g}")
    assert status == 0
    assert r_t <= 1.0 and r_T <= 1.0
    assert np.array_equal(_bits(T[:3, 3]), _bits(t[3:]))
    Rm = T[:3, :3]
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(Rm) - 1.0) <= 1e-12


@pytest.mark.gpu
def test_solve_status_bits():
    from pings_amd import _abi

    g = np.array([0.01, -0.02, 0.03, 0.1, 0.2, -0.3])
    sys_ = lambda N, rhs=g: np.concatenate([np.asarray(N, np.float64).ravel(), rhs])
    diag = lambda last: np.diag([1.0, 1.0, 1.0, 1.0, 1.0, last])
    # the ill-conditioning threshold from both sides: smallest pivot / largest entry 2e-7 and 5e-8 against 1e-7
    assert _solve(sys_(diag(2e-7)), 0.0)[2] == 0
    assert _solve(sys_(diag(5e-8)), 0.0)[2] == _abi.REG_ILL_CONDITIONED
    zero = _spd(10.0, 1).astype(np.float64)
    zero[2, :] = 0.0
    zero[:, 2] = 0.0
    assert _solve(sys_(zero), 0.0)[2] & _abi.REG_SINGULAR
    inf = _spd(10.0, 1).astype(np.float64)
    inf[4, 4] = np.inf
    assert _solve(sys_(inf), 0.0)[2] & _abi.REG_SINGULAR
    # g = 0: t = 0, the axis of the exponential map is 0 / 0 as in the reference: non-finite, not singular
    T, t, status = _solve(sys_(_spd(10.0, 1), np.zeros(6)), 0.0)
    assert status & _abi.REG_NONFINITE and not status & _abi.REG_SINGULAR and np.all(t == 0.0) and np.isnan(T[0, 0])
