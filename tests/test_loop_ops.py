"""Global loop detection on the device (pings_amd/loop_ops.py, csrc/loop.hip) against the reference.

Three yardsticks (tests/loop_ref.py): tests/golden/loop_*.npz from the reference's own functions and manager
(tools/make_loop_golden.py), the fp32 restatement that equals them exactly on the CPU, and the fp64 judge.

Bounds, none of them measured: a bin fp32 cannot decide (loop_ref: decidability) is left out, at most 1 % of a case's
bins, none in the filtered family; `sc` in the sensor frame is bit-equal to fp64 rounded once; under a virtual pose it is
within e = 4 * 2^-23 * (|p|_1 + |t|_1) of the winning point (a neighbour of the winner in the same bin can overtake it
only by its own rounding error, which is below the winner's e as long as |p|_1 + |t|_1 does not vary by a factor 2.6
inside a bin); feature means within (n + 2) * 2^-23 * max|f|; ring keys the same plus S * 2^-23 * max|value|.  Search:
the fp64 margins of the winner (1e-3 of the largest ring-key distance, 1e-4 between shift means) are asserted on the
CPU, so indices agree exactly; distances within (R + S * D + 8) * 2^-23 * max(1, |d|).

The fp32 restatement against the fixtures, on the CPU: everything whose arithmetic has one order is compared with
array_equal (bins, maxima, feature means, which torch adds in index order, offsets, the loop, the shift, the 4x4
result).  torch's horizontal CPU reductions (`mean` over the sectors, the norms and means inside the cosine distances)
add in an order that depends on the vector width of the CPU they run on, so a ring key is compared within what two
orders of one fp32 sum of S terms can differ by, S * 2^-23 * max|value|, and a cosine distance within twice the bound
above; on the CPU that wrote the fixtures both differences are zero.
"""
import ctypes as C
import functools
import struct
import types

import numpy as np
import pytest
import torch

import loop_ref as LR

# (n, M, D, shape, filtered, variant)
_SHAPES = ((20, 60), (3, 7))
BUILD_CASES = [(n, M, D, shape, not (n == 20000 and shape == (20, 60)), "beyond" if n == 0 else "field")
               for n in (0, 1, 63, 64, 65, 257, 4097, 20000) for M in (1, 11) for D in (0, 8) for shape in _SHAPES]
BUILD_CASES += [(4097, M, 8, (20, 60), True, v) for M in (1, 11) for v in ("below", "nonfinite")]
# (C, Q, use_feature, tie)
SEARCH_CASES = [(Cn, Q, f, None) for Cn in (1, 2, 64, 65, 1025) for Q in (1, 11) for f in (False, True)]
SEARCH_CASES += [(65, 11, f, t) for f in (False, True) for t in ("slot", "query", "period")]


def _id(case):
    return "-".join(str(c).replace(" ", "") for c in case)


@functools.lru_cache(maxsize=None)
def build_case(case):
    n, M, D, shape, filtered, variant = case
    pts, f, T, max_length = LR.context_case(257 if variant == "beyond" else n, M, D, shape, filtered,
                                            seed=n + 3 * M + D, variant=variant)
    return pts, f, T, max_length, LR.judge_contexts(pts, f, T, shape[0], shape[1], max_length)


@functools.lru_cache(maxsize=None)
def search_case(case):
    Cn, Q, feature, tie = case
    c = LR.search_case(Cn, Q, feature, seed=Cn + Q, slots=Cn + Cn // 2 + 5, tie=tie)
    return c, LR.judge_search(c["ctx"], c["key"], c["cand"], c["q_ctx"], c["q_key"], feature)


def _same_mean(got, want, src, S):
    """`got` and `want` are fp32 means over the S sectors (dim 1) of `src`, possibly added in different orders."""
    tol = S * LR.U * np.abs(np.asarray(src, dtype=np.float64)).max(axis=1)
    return bool((np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)) <= tol).all())


def _same_dist(got, want, shape):
    R, S = shape[0], shape[1]
    return abs(got - want) <= 2 * LR.distance_tol(R, S, shape[2] if len(shape) == 3 else 0, want)


def _standin():
    """A module shaped like utils.loop_detector, with a manager class of its own to rebind."""
    return types.SimpleNamespace(
        ptcloud2sc_torch=LR.ptcloud2sc_torch, sc2rk=LR.sc2rk, distance_sc_torch=LR.distance_sc_torch,
        distance_sc_feature_torch=LR.distance_sc_feature_torch,
        NeuralPointMapContextManager=type("NeuralPointMapContextManager", (LR.NeuralPointMapContextManager,), {}))


@pytest.fixture
def installed():
    from pings_amd import loop_ops

    mod = _standin()
    loop_ops.install(mod)
    try:
        yield mod
    finally:
        loop_ops.uninstall(mod)


# ================================================================ CPU: restatement, judge, caps
def test_fp32_restatement_equals_the_context_fixture():
    fix = LR.load("loop_context.npz")
    pts, feats = torch.from_numpy(fix["points"]), torch.from_numpy(fix["features"].astype(np.float32))
    for tag in "ab":
        shape = [int(v) for v in fix[f"shape_{tag}"]]
        sc, scf = LR.ptcloud2sc_torch(pts, feats, shape, float(fix["max_length"]))
        assert np.array_equal(sc.numpy(), fix[f"sc_{tag}"]) and np.array_equal(scf.numpy(), fix[f"scf_{tag}"])
        assert _same_mean(LR.sc2rk(sc).numpy(), fix[f"rk_{tag}"], sc.numpy(), shape[1])
        assert _same_mean(LR.sc2rk(scf).numpy(), fix[f"rkf_{tag}"], scf.numpy(), shape[1])


def test_fp64_judge_agrees_with_the_context_fixture():
    fix = LR.load("loop_context.npz")
    pts, feats = torch.from_numpy(fix["points"]), torch.from_numpy(fix["features"].astype(np.float32))
    for tag in "ab":
        R, S = [int(v) for v in fix[f"shape_{tag}"]]
        J = LR.judge_contexts(pts, feats, LR.IDENTITY, R, S, float(fix["max_length"]))
        got = tuple(torch.from_numpy(fix[f"{k}_{tag}"]).unsqueeze(0) for k in ("sc", "rk", "scf", "rkf"))
        assert LR.check_contexts(got, J, True, S) > 0


def _distance_pairs():
    fix = LR.load("loop_distance.npz")
    for i in range(int(fix["count"])):
        a, b = (torch.from_numpy(fix[f"{k}_{i}"].astype(np.float32)) for k in "ab")
        yield a, b, float(fix[f"dist_{i}"]), int(fix[f"yaw_{i}"])


def test_restatements_agree_with_the_distance_fixture():
    for a, b, dist, yaw in _distance_pairs():
        f = LR.distance_sc_feature_torch if a.dim() == 3 else LR.distance_sc_torch
        d, y = f(a, b)
        assert y == yaw and _same_dist(d, dist, a.shape)
        J = LR.judge_search(a.unsqueeze(0), a.mean(dim=1).unsqueeze(0), [0], b.unsqueeze(0), b.mean(dim=1).unsqueeze(0),
                            a.dim() == 3)
        assert J["shift_margin"] > 1e-4 and J["shift"] == yaw
        assert abs(J["cos"] - dist) <= LR.distance_tol(a.shape[0], a.shape[1], a.shape[2] if a.dim() == 3 else 0, J["cos"])


@pytest.mark.parametrize("use_feature", [False, True])
def test_fp32_restatement_equals_the_sequence_fixture(use_feature):
    fix = LR.load("loop_sequence.npz")
    tag = "feature" if use_feature else "plain"
    mgr, (loop_id, cosdist, T) = LR.run_sequence(LR, fix, use_feature)
    shape = (20, 60, 8) if use_feature else (20, 60)
    assert loop_id == int(fix[f"loop_id_{tag}"]) and _same_dist(cosdist, float(fix[f"cosdist_{tag}"]), shape)
    assert np.array_equal(T, fix[f"T_{tag}"])
    keys = mgr.ringkeys_feature if use_feature else mgr.ringkeys
    ctxs = mgr.contexts_feature if use_feature else mgr.contexts
    for k, i in enumerate(int(i) for i in fix["frame_ids"]):
        assert _same_mean(keys[i].numpy(), fix[f"ringkeys_{tag}"][k], ctxs[i].numpy(), 60)
    assert np.array_equal(torch.stack(mgr.tran_from_frame).numpy(), fix[f"tran_from_frame_{tag}"])
    for k, qc in enumerate(mgr.query_contexts):
        assert _same_mean(LR.sc2rk(qc).numpy(), fix[f"query_ringkeys_{tag}"][k], qc.numpy(), 60)
    if not use_feature:
        assert np.array_equal(mgr.contexts[0].numpy(), fix["context0_plain"])
    # the decision margins of the sequence, in fp64, on the descriptors the restatement built
    ids = [int(i) for i in fix["frame_ids"]]
    bank_ctx, bank_key = torch.stack([ctxs[i] for i in ids]), torch.stack([keys[i] for i in ids])
    cand = [ids.index(int(c)) for c in fix["candidates"]]
    q_ctx = torch.stack(mgr.query_contexts)
    J = LR.judge_search(bank_ctx, bank_key, cand, q_ctx, q_ctx.mean(dim=2), use_feature)
    assert J["rk_margin"] > 1e-3 and J["shift_margin"] > 1e-4
    assert ids[cand[J["cpos"]]] == loop_id


def test_every_point_of_the_sequence_is_decidable():
    fix = LR.load("loop_sequence.npz")
    pts, _, poses = LR.sequence_inputs(fix)
    for k in range(poses.shape[0]):
        assert not LR.undecidable_points(LR.to_sensor(pts, poses[k]), LR.IDENTITY, 20, 60, 60.0).any()
    T, _, _ = LR.virtual_transforms(poses[-1], poses[-2], 5, 2.0)
    assert not LR.undecidable_points(pts, T, 20, 60, 60.0).any()


@pytest.mark.parametrize("case", BUILD_CASES, ids=_id)
def test_left_out_bins_stay_under_the_cap(case):
    n, M, D, shape, filtered, variant = case
    pts, f, T, max_length, J = build_case(case)
    left = int(J["left_out"].sum())
    if filtered:
        assert left == 0
    else:
        assert left <= 0.01 * J["left_out"].numel()
    if variant == "beyond":
        assert int(J["n"].sum()) == 0
    elif n >= 63:
        assert int(J["n"].sum()) > 0
    if variant == "below":
        assert float(J["sc"].max()) == 0.0 and float(J["sc"].min()) < 0.0


@pytest.mark.parametrize("case", SEARCH_CASES, ids=_id)
def test_search_cases_have_decision_margins(case):
    Cn, Q, feature, tie = case
    c, J = search_case(case)
    assert J["rk_margin"] > 1e-3 and J["shift_margin"] > 1e-4
    assert (J["cpos"], J["q"], J["shift"]) == (c["cw"], c["qw"], c["shift"])
    if tie == "slot":
        assert sum(np.array_equal(c["key"][s].numpy(), c["key"][c["cand"][c["cw"]]].numpy()) for s in c["cand"]) == 2
    if tie == "query":
        assert torch.equal(c["q_ctx"][-1], c["q_ctx"][c["qw"]])
    if tie == "period":
        other = c["shift"] + c["S"] // 2
        assert abs(float(J["sims"][other - 1]) - float(J["sims"][c["shift"] - 1])) <= LR.TIE   # a tie, the smaller wins


# ================================================================ CPU: ABI, status codes, install
LOOP_ENTRIES = ("pings_loop_context_scratch_bytes", "pings_loop_context_build", "pings_loop_ring_key",
                "pings_loop_virtual_poses", "pings_loop_search", "pings_loop_context_distance",
                "pings_loop_read_record")


def test_symbols_are_declared_exported_and_typed():
    import abi_header as hdr
    from pings_amd import _abi, _lib, loop_ops

    L = _lib.lib()
    protos = hdr.prototypes()
    for name in LOOP_ENTRIES:
        assert name in protos and name in _abi.SIGNATURES and hasattr(L, name)
        restype, argtypes = _abi.SIGNATURES[name]
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes)
        assert len(argtypes) == len(protos[name][1])
    for name in ("scan_context", "ring_key", "context_distance", "add_node", "set_virtual_node", "detect_loop",
                 "install", "uninstall", "build_contexts", "LIMITS"):
        assert hasattr(loop_ops, name)
    assert loop_ops.LIMITS["R"] >= 20 and loop_ops.LIMITS["S"] >= 60 and loop_ops.LIMITS["D"] >= 8
    assert loop_ops.LIMITS["Q"] >= 11 and loop_ops.LIMITS["C"] >= 4096


def test_null_pointers_and_shapes_over_the_limits_are_status_codes():
    from pings_amd import _abi, _lib

    L = _lib.lib()
    one = C.c_void_p(1).value                       # never dereferenced: every call below fails its argument check
    st = L.pings_loop_context_build(None, 10, None, 0, None, 1, 20, 60, 60.0, None, None, None, None, None, None, None,
                                    None, None, None, None)
    assert st == 1 and b"null" in L.pings_last_error()
    st = L.pings_loop_context_build(one, 10, None, 0, one, 1, _abi.LOOP_MAX_R + 1, 60, 60.0, None, None, None, None,
                                    None, one, one, one, None, None, None)
    assert st == 1 and b"limits" in L.pings_last_error()
    st = L.pings_loop_context_build(one, 10, None, 0, one, _abi.LOOP_MAX_Q + 1, 20, 60, 60.0, None, None, None, None,
                                    None, one, one, one, None, None, None)
    assert st == 1 and b"limits" in L.pings_last_error()
    assert L.pings_loop_context_scratch_bytes(10, 1, 20, _abi.LOOP_MAX_S + 1, 0) == 0
    assert L.pings_loop_context_scratch_bytes(10, 11, 20, 60, 8) > 0
    st = L.pings_loop_search(None, None, 4, None, 1, None, None, 1, 20, 60, 0, 0, 1.0, None, None, None, None)
    assert st == 1 and b"null" in L.pings_last_error()
    st = L.pings_loop_search(one, one, 4, one, _abi.LOOP_MAX_C + 1, one, one, 1, 20, 60, 0, 0, 1.0, None, one, None, None)
    assert st == 1 and b"limits" in L.pings_last_error()
    st = L.pings_loop_search(one, one, 4, one, 1, one, one, 1, 20, 60, _abi.LOOP_MAX_D + 1, 1, 1.0, None, one, None, None)
    assert st == 1 and b"limits" in L.pings_last_error()
    assert L.pings_loop_virtual_poses(None, None, 5, 2.0, None, None, None, None, None) == 1
    assert L.pings_loop_virtual_poses(one, None, 8, 2.0, one, one, one, one, None) == 1
    assert L.pings_loop_ring_key(None, 20, 60, 0, None, None) == 1
    assert L.pings_loop_context_distance(None, None, 20, 60, 0, None, None) == 1
    assert L.pings_loop_read_record(None, None, None, None) == 1


def test_install_and_uninstall_round_trip():
    from pings_amd import loop_ops

    mod = _standin()
    before = {k: getattr(mod, k) for k in ("ptcloud2sc_torch", "sc2rk", "distance_sc_torch", "distance_sc_feature_torch")}
    cls = mod.NeuralPointMapContextManager
    loop_ops.install(mod)
    loop_ops.install(mod)                            # twice changes nothing
    assert mod.ptcloud2sc_torch is loop_ops.scan_context and mod.sc2rk is loop_ops.ring_key
    assert mod.distance_sc_torch is loop_ops.context_distance is mod.distance_sc_feature_torch
    assert cls.add_node is loop_ops.add_node and cls.detect_loop is loop_ops.detect_loop
    assert cls.set_virtual_node is loop_ops.set_virtual_node
    assert cls._pings_add_node_original is LR.NeuralPointMapContextManager.add_node
    loop_ops.uninstall(mod)
    assert {k: getattr(mod, k) for k in before} == before
    for name in ("add_node", "set_virtual_node", "detect_loop"):
        assert getattr(cls, name) is getattr(LR.NeuralPointMapContextManager, name)
        assert not hasattr(cls, f"_pings_{name}_original")


@pytest.mark.parametrize("use_feature", [False, True])
def test_cpu_tensors_reach_the_kept_originals(installed, use_feature):
    from pings_amd import loop_ops

    fix = LR.load("loop_sequence.npz")
    tag = "feature" if use_feature else "plain"
    mgr, (loop_id, cosdist, T) = LR.run_sequence(installed, fix, use_feature)
    assert type(mgr).add_node is loop_ops.add_node
    assert loop_id == int(fix[f"loop_id_{tag}"])
    assert _same_dist(cosdist, float(fix[f"cosdist_{tag}"]), (20, 60, 8) if use_feature else (20, 60))
    assert np.array_equal(T, fix[f"T_{tag}"])
    assert mgr.detect_loop(np.zeros(0, dtype=np.int64)) == (None, None, None)
    ctx = LR.load("loop_context.npz")
    pts = torch.from_numpy(ctx["points"])
    sc, scf = installed.ptcloud2sc_torch(pts, None, [20, 60], 60.0)
    assert scf is None and np.array_equal(sc.numpy(), ctx["sc_a"])
    assert _same_mean(installed.sc2rk(sc).numpy(), ctx["rk_a"], sc.numpy(), 60)
    assert installed.ptcloud2sc_torch(pts.double(), None, [20, 60], 60.0)[0].dtype is torch.float64
    for a, b, dist, yaw in _distance_pairs():
        d, y = (installed.distance_sc_feature_torch if a.dim() == 3 else installed.distance_sc_torch)(a, b)
        assert y == yaw and _same_dist(d, dist, a.shape)


def test_without_an_original_other_inputs_raise():
    from pings_amd import _lib, loop_ops

    with pytest.raises(_lib.PingsHipError, match="none was kept"):
        loop_ops.scan_context(torch.zeros(4, 3), None, [20, 60], 60.0)


# ================================================================ GPU: build
def _gpu_build(case):
    from pings_amd import loop_ops

    pts, f, T, max_length, J = build_case(case)
    dev = "cuda"
    args = (pts.to(dev), None if f is None else f.to(dev), T.to(dev), case[3], max_length)
    a = loop_ops.build_contexts(*args)
    b = loop_ops.build_contexts(*args)
    cpu = lambda out: tuple(None if t is None else t.cpu() for t in out)  # noqa: E731
    return cpu(a), cpu(b), J


@pytest.mark.gpu
@pytest.mark.parametrize("case", BUILD_CASES, ids=_id)
def test_build_against_fp64(case):
    n, M, D, shape, filtered, variant = case
    a, b, J = _gpu_build(case)
    for x, y in zip(a, b):                           # two runs agree bit for bit
        assert (x is None and y is None) or torch.equal(x, y)
    assert a[0].shape == (M, *shape) and a[1].shape == (M, shape[0])
    if D:
        assert a[2].shape == (M, *shape, D) and a[3].shape == (M, shape[0], D)
    compared = LR.check_contexts(a, J, M == 1, shape[1])
    assert compared >= 0.99 * J["left_out"].numel()
    if variant == "beyond":
        assert all(t is None or not t.any() for t in a)
    if variant == "below":
        assert float(a[0].min()) < 0.0 and float(a[0].max()) == 0.0     # negative maxima kept, empty bins 0.0
        assert bool((a[0][J["n"] > 0] < 0).all())


@pytest.mark.gpu
def test_a_point_at_exactly_max_length_is_dropped():
    from pings_amd import loop_ops

    # r is exactly 60 in fp32 for the first three (36^2 + 48^2 = 60^2); the fourth stays 4 ulp inside
    pts = torch.tensor([[60.0, 0.0, 0.0], [0.0, -60.0, 0.0], [36.0, 48.0, 0.0], [59.99999, 0.0, 0.001], [1.0, 1.0, 2.0]],
                       device="cuda")
    sc, scf = loop_ops.scan_context(pts, None, [20, 60], 60.0)
    assert scf is None
    want, _ = LR.ptcloud2sc_torch(pts.cpu(), None, [20, 60], 60.0)
    assert torch.equal(sc.cpu(), want) and int((want != 0).sum()) == 2
    assert float(want[19].max()) == float(np.float32(0.001)) and float(want[0].max()) == 2.0


@pytest.mark.gpu
def test_module_functions_on_the_device_against_the_fixtures():
    from pings_amd import loop_ops

    ctx = LR.load("loop_context.npz")
    pts, feats = torch.from_numpy(ctx["points"]).cuda(), torch.from_numpy(ctx["features"].astype(np.float32)).cuda()
    for tag in "ab":
        R, S = [int(v) for v in ctx[f"shape_{tag}"]]
        J = LR.judge_contexts(pts.cpu(), feats.cpu(), LR.IDENTITY, R, S, 60.0)
        sc, scf = loop_ops.scan_context(pts, feats, [R, S], 60.0)
        rk, rkf = loop_ops.ring_key(sc), loop_ops.ring_key(scf)
        got = tuple(t.cpu().unsqueeze(0) for t in (sc, rk, scf, rkf))
        LR.check_contexts(got, J, True, S)
        keep = ~J["left_out"][0]
        assert np.array_equal(sc.cpu().numpy()[keep.numpy()], ctx[f"sc_{tag}"][keep.numpy()])
    for a, b, dist, yaw in _distance_pairs():
        d, s = loop_ops.context_distance(a.cuda(), b.cuda())
        assert s == yaw and isinstance(d, float) and isinstance(s, int)
        assert abs(d - dist) <= 2 * LR.distance_tol(a.shape[0], a.shape[1], a.shape[2] if a.dim() == 3 else 0, dist)


# ================================================================ GPU: search
SENTINEL = 0x7777


def _gpu_search(c, thre):
    from pings_amd import _lib
    from pings_amd.pool_ops import _entry

    dev = torch.device("cuda", torch.cuda.current_device())
    t = {k: c[k].to(dev) for k in ("ctx", "key", "q_ctx", "q_key")}
    cand = torch.from_numpy(c["cand"]).to(dev)
    record = torch.full((8,), SENTINEL, dtype=torch.int32, device=dev)
    _lib.check(_entry("pings_loop_search")(
        t["ctx"].data_ptr(), t["key"].data_ptr(), int(c["ctx"].shape[0]), cand.data_ptr(), int(cand.shape[0]),
        t["q_ctx"].data_ptr(), t["q_key"].data_ptr(), int(c["q_ctx"].shape[0]), c["R"], c["S"], c["D"],
        int(c["use_feature"]), float(thre), None, record.data_ptr(), None, _lib.stream_ptr(dev)), "pings_loop_search")
    raw = record.cpu().numpy().tobytes()
    return struct.unpack("<iiffiiii", raw)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SEARCH_CASES, ids=_id)
def test_search_against_fp64(case):
    c, J = search_case(case)
    cpos, q, rk, cos, shift, gate, s6, s7 = _gpu_search(c, 1e4)
    assert (cpos, q, shift, gate) == (J["cpos"], J["q"], J["shift"], 1)
    assert (s6, s7) == (SENTINEL, SENTINEL)
    assert abs(rk - J["rk"]) <= LR.distance_tol(c["R"], c["S"], c["D"], J["rk"])
    assert abs(cos - J["cos"]) <= LR.distance_tol(c["R"], c["S"], c["D"], J["cos"])


@pytest.mark.gpu
@pytest.mark.parametrize("feature", [False, True])
def test_a_closed_ringkey_gate_leaves_phase_two_untouched(feature):
    c, J = search_case((65, 11, feature, None))
    cpos, q, rk, cos, shift, gate, _, _ = _gpu_search(c, J["rk"] - max(0.5 * J["rk"], 1e-3))
    assert (cpos, q, gate) == (J["cpos"], J["q"], 0)
    assert abs(rk - J["rk"]) <= LR.distance_tol(c["R"], c["S"], c["D"], J["rk"])
    assert struct.pack("<f", cos) == struct.pack("<i", SENTINEL) and shift == SENTINEL
    assert _gpu_search(c, J["rk"] + max(J["rk"], 1e-3))[5] == 1


# ================================================================ GPU: the manager
@pytest.mark.gpu
@pytest.mark.parametrize("use_feature", [False, True])
def test_manager_sequence_against_the_fixture(installed, use_feature):
    from pings_amd import _lib

    fix = LR.load("loop_sequence.npz")
    tag = "feature" if use_feature else "plain"
    _lib.sync_counts(reset=True)
    mgr, (loop_id, cosdist, T) = LR.run_sequence(installed, fix, use_feature, device="cuda")
    assert _lib.sync_counts() == {"loop_detect": 1}
    tol = 2 * LR.distance_tol(20, 60, 8 if use_feature else 0, 1.0)
    assert loop_id == int(fix[f"loop_id_{tag}"]) and isinstance(loop_id, int) and isinstance(cosdist, float)
    assert abs(cosdist - float(fix[f"cosdist_{tag}"])) <= tol
    # the offsets are fp32 values of up to 10 m formed from an fp64 direction: one fp32 ulp of slack, 2^-20 m
    assert isinstance(T, np.ndarray) and T.dtype == np.float64 and np.abs(T - fix[f"T_{tag}"]).max() <= 2.0 ** -20
    # the lists are views of the bank, also after it grew (frame ids run past its first 64 rows)
    bank = mgr._pings_bank
    assert bank.cap > 64
    ids = [int(i) for i in fix["frame_ids"]]
    keys = mgr.ringkeys_feature if use_feature else mgr.ringkeys
    ctxs = mgr.contexts_feature if use_feature else mgr.contexts
    for i in ids:
        assert ctxs[i]._base is (bank.scf if use_feature else bank.sc) and keys[i]._base is not None
        assert mgr.contexts[i]._base is bank.sc
    got_keys = torch.stack([keys[i] for i in ids]).cpu().numpy()
    assert np.abs(got_keys - fix[f"ringkeys_{tag}"]).max() <= 60 * LR.U * np.abs(fix[f"ringkeys_{tag}"]).max() * 2
    assert np.array_equal(mgr.contexts[0].cpu().numpy(), fix["context0_plain"])       # sensor frame: bit-equal
    assert len(mgr.query_contexts) == 11 == len(mgr.tran_from_frame)
    assert np.abs(torch.stack(list(mgr.tran_from_frame)).cpu().numpy() - fix[f"tran_from_frame_{tag}"]).max() <= 2.0 ** -20
    q_keys = torch.stack([LR.sc2rk(qc.cpu()) for qc in mgr.query_contexts]).numpy()
    assert np.abs(q_keys - fix[f"query_ringkeys_{tag}"]).max() <= 1e-4
    assert torch.equal(mgr.query_contexts[5], ctxs[ids[-1]])                          # the centre: the stored descriptor
    # the cosine threshold on either side of what was found
    mgr.sc_cosdist_threshold = cosdist + 1e-3
    assert mgr.detect_loop(fix["candidates"], use_feature=use_feature)[0] == loop_id
    mgr.sc_cosdist_threshold = cosdist - 1e-3
    assert mgr.detect_loop(fix["candidates"], use_feature=use_feature) == (None, None, None)
    mgr.sc_cosdist_threshold, keep = cosdist + 1e-3, mgr.ringkey_dist_thre
    mgr.ringkey_dist_thre = 1e-9
    assert mgr.detect_loop(fix["candidates"], use_feature=use_feature) == (None, None, None)
    mgr.ringkey_dist_thre = keep
    assert mgr.detect_loop(np.zeros(0, dtype=np.int64), use_feature=use_feature) == (None, None, None)


@pytest.mark.gpu
@pytest.mark.parametrize("use_feature", [False, True])
def test_detect_loop_without_virtual_nodes_uses_the_current_node(installed, use_feature):
    fix = LR.load("loop_sequence.npz")
    pts, feats, poses = LR.sequence_inputs(fix)
    out = []
    for dev, module in (("cpu", LR), ("cuda", installed)):
        cfg = LR.make_config(device=dev, end_frame=100, loop_with_feature=use_feature, local_map_context=True,
                             context_cosdist_threshold=2.0)
        mgr = module.NeuralPointMapContextManager(cfg)
        mgr.ringkey_dist_thre = 1e4
        for k in (0, 3, 11):
            mgr.add_node(k, LR.to_sensor(pts, poses[k]).to(dev), feats.to(dev) if use_feature else None)
        out.append(mgr.detect_loop(np.array([3, 0]), use_feature=use_feature))
        assert len(mgr.query_contexts) == 1 and torch.equal(mgr.tran_from_frame[0].cpu(), torch.eye(4, dtype=torch.float64))
    (id0, d0, T0), (id1, d1, T1) = out
    assert id0 == id1 and np.array_equal(T0, T1)          # no lateral offset here: the yaw matrix alone
    assert abs(d0 - d1) <= 2 * LR.distance_tol(20, 60, 8 if use_feature else 0, 1.0)


@pytest.mark.gpu
def test_host_reads_one_for_detect_loop_none_for_the_rest(installed):
    from pings_amd import _lib

    fix = LR.load("loop_sequence.npz")
    pts, feats, poses = LR.sequence_inputs(fix)
    LR.run_sequence(installed, fix, True, device="cuda")             # warm-up: loads the library, fills the caches
    dev = "cuda"
    cfg = LR.make_config(device=dev, end_frame=100, loop_with_feature=True, local_map_context=True)
    mgr = installed.NeuralPointMapContextManager(cfg)
    ids = [int(i) for i in fix["frame_ids"]]
    clouds = [LR.to_sensor(pts, poses[k]).to(dev) for k in range(len(ids))]
    world, f_dev, p_cur, p_last = pts.to(dev), feats.to(dev), poses[-1].to(dev), poses[-2].to(dev)
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    _lib.sync_counts(reset=True)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                            # positive control: the mode catches a read
            probe.sum().item()
        for i, cloud in zip(ids, clouds):                            # grows the bank on the way
            mgr.add_node(i, cloud, f_dev)
        mgr.set_virtual_node(world, p_cur, p_last, f_dev)
        assert _lib.sync_counts() == {}
        triple = mgr.detect_loop(fix["candidates"], use_feature=True)
        assert _lib.sync_counts() == {"loop_detect": 1}
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert triple[0] == int(fix["loop_id_feature"])


@pytest.mark.gpu
def test_identical_consecutive_poses_give_what_the_reference_gives(installed):
    """0 / 0 in the direction of travel: NaN offsets, every point dropped, all-zero descriptors, NaN in tran_from_frame.
    The device path reproduces it (no host wait to detect the case); compared with the restatement on the CPU."""
    fix = LR.load("loop_sequence.npz")
    pts, _, poses = LR.sequence_inputs(fix)
    out = []
    for dev, module in (("cpu", LR), ("cuda", installed)):
        mgr = module.NeuralPointMapContextManager(LR.make_config(device=dev, end_frame=100))
        mgr.add_node(2, LR.to_sensor(pts, poses[0]).to(dev))
        mgr.set_virtual_node(pts.to(dev), poses[0].to(dev), poses[0].clone().to(dev))
        out.append((torch.stack(list(mgr.query_contexts)).cpu(), torch.stack(list(mgr.tran_from_frame)).cpu()))
    (q0, t0), (q1, t1) = out
    assert q0.shape == q1.shape == (11, 20, 60) and not q0.any() and not q1.any()
    assert torch.equal(torch.isnan(t0), torch.isnan(t1)) and bool(torch.isnan(t1[:, :3, 3]).all())
    assert torch.equal(torch.nan_to_num(t0), torch.nan_to_num(t1))
