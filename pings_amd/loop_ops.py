"""Global loop detection on the HIP device (csrc/loop.hip).

Drop-ins for utils/loop_detector.py of the reference, by the reference's own names and on its own objects:

  `scan_context`      `ptcloud2sc_torch`: (sc [R,S], sc_feature [R,S,D] or None) from a cloud in its sensor frame
  `ring_key`          `sc2rk`
  `context_distance`  `distance_sc_torch` / `distance_sc_feature_torch` (the arguments' dimension picks which): two python
                      numbers after one host read
  `add_node`, `set_virtual_node`, `detect_loop`   the three methods of `NeuralPointMapContextManager`

The manager's descriptors live in a device bank indexed by frame id that grows geometrically; `contexts[i]`,
`ringkeys[i]` and the `_feature` lists stay what they were, tensors one can read: views of the bank's rows, rebound
when the bank grows.  `detect_loop` makes one host read (the search record); `add_node` and `set_virtual_node` make
none.  `install` rebinds the three module functions and the three methods and keeps the originals, which take the
inputs the kernels do not (CPU tensors, non-float32 clouds, shapes outside `LIMITS`).  There is no torch path of this
module's own: with no original kept, such a call raises.

The reference's quirks are kept: an empty bin is 0.0, the centre virtual pose takes the node's stored
descriptor, the shift is reported in 1..S (S = no rotation).
"""
from __future__ import annotations

import ctypes as C
import math
import struct

import numpy as np
import torch

from . import _abi, _lib
from .pool_ops import _entry, _f32_dev, _guard

LIMITS = {"R": _abi.LOOP_MAX_R, "S": _abi.LOOP_MAX_S, "D": _abi.LOOP_MAX_D, "Q": _abi.LOOP_MAX_Q,
          "C": _abi.LOOP_MAX_C}
_BANK_MIN = 64                       # rows of a new bank
_FUNCTIONS = (("ptcloud2sc_torch", "scan_context"), ("sc2rk", "ring_key"), ("distance_sc_torch", "context_distance"),
              ("distance_sc_feature_torch", "context_distance"))
_originals: dict = {}                # reference function name -> the module's own function (kept by `install`)
_identity: dict = {}                 # device -> [1,12] float32 identity transform


def _original_fn(name: str):
    fn = _originals.get(name)
    if fn is None:
        raise _lib.PingsHipError(f"loop_ops: these inputs take the reference's own {name}, and none was kept "
                                 "(`loop_ops.install` keeps it); the HIP path needs contiguous float32 device tensors "
                                 f"and a shape inside {LIMITS}")
    return fn


def _original(self, name: str):
    orig = getattr(type(self), f"_pings_{name}_original", None)
    if orig is None:
        raise _lib.PingsHipError(f"loop_ops.{name}: these inputs take the reference's own method, and none was kept "
                                 "(`loop_ops.install` keeps it); the HIP path needs contiguous float32 device tensors "
                                 f"and a shape inside {LIMITS}")
    return orig


def _shape_ok(R, S, D=0) -> bool:
    return 1 <= R <= LIMITS["R"] and 1 <= S <= LIMITS["S"] and 0 <= D <= LIMITS["D"]


def _cloud_ok(pts, feats) -> bool:
    if not (_f32_dev(pts) and pts.dim() == 2 and pts.shape[1] == 3):
        return False
    return feats is None or (_f32_dev(feats, pts.device) and feats.dim() == 2 and feats.shape[0] == pts.shape[0]
                             and 1 <= feats.shape[1] <= LIMITS["D"])


def _eye12(dev) -> torch.Tensor:
    t = _identity.get(dev)
    if t is None:
        t = _identity[dev] = torch.eye(3, 4, dtype=torch.float32, device=dev).reshape(1, 12).contiguous()
    return t


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


@torch.no_grad()
def build_contexts(points, features, transforms, sc_shape, max_length, out=None, stored=None):
    """Descriptors of the M poses `transforms` [M,12] (float32, row-major 3x4) of one cloud: (sc [M,R,S], ringkey [M,R],
    sc_feature [M,R,S,D] | None, ringkey_feature [M,R,D] | None).  `out` takes the same four as preallocated
    contiguous tensors; `stored` = (use_stored [M] int32 on the device, sc, ringkey, sc_feature, ringkey_feature) makes
    the flagged poses copies of one stored descriptor.  One library call, no host read."""
    R, S = int(sc_shape[0]), int(sc_shape[1])
    dev = points.device
    M, N = int(transforms.shape[0]), int(points.shape[0])
    D = 0 if features is None else int(features.shape[1])
    if not (_cloud_ok(points, features) and _f32_dev(transforms, dev) and _shape_ok(R, S, D) and 1 <= M <= LIMITS["Q"]):
        raise _lib.PingsHipError("loop_ops.build_contexts: points [N,3], features [N,D] and transforms [M,12] must be "
                                 f"contiguous float32 tensors on one HIP device, inside {LIMITS}")
    with _guard(dev):
        if out is None:
            e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
            out = (e(M, R, S), e(M, R), e(M, R, S, D) if D else None, e(M, R, D) if D else None)
        sc, rk, scf, rkf = out
        nbytes = _entry("pings_loop_context_scratch_bytes")(N, M, R, S, D)
        if nbytes == 0:
            raise _lib.PingsHipError(f"loop_ops.build_contexts: {N} points x {M} poses is outside the kernels' range")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        st = stored if stored is not None else (None,) * 5
        _lib.check(_entry("pings_loop_context_build")(
            _ptr(points), N, _ptr(features), D, transforms.data_ptr(), M, R, S, float(max_length), _ptr(st[0]),
            _ptr(st[1]), _ptr(st[2]), _ptr(st[3]) if D else None, _ptr(st[4]) if D else None, scratch.data_ptr(),
            sc.data_ptr(), rk.data_ptr(), _ptr(scf), _ptr(rkf), _lib.stream_ptr(dev)), "pings_loop_context_build")
    return sc, rk, scf, rkf


# ---------------------------------------------------------------- the module functions
def scan_context(ptcloud, pt_feature, sc_shape, max_length):
    """`ptcloud2sc_torch`: (sc [R,S], sc_feature [R,S,D] or None)."""
    R, S = int(sc_shape[0]), int(sc_shape[1])
    if not (_cloud_ok(ptcloud, pt_feature) and _shape_ok(R, S)):
        return _original_fn("ptcloud2sc_torch")(ptcloud, pt_feature, sc_shape, max_length)
    sc, _, scf, _ = build_contexts(ptcloud, pt_feature, _eye12(ptcloud.device), (R, S), max_length)
    return sc[0], (None if scf is None else scf[0])


@torch.no_grad()
def ring_key(sc):
    """`sc2rk`: the mean over the sectors, in ascending sector."""
    if not (_f32_dev(sc) and sc.dim() in (2, 3) and _shape_ok(sc.shape[0], sc.shape[1], sc.shape[2] if sc.dim() == 3 else 0)
            and (sc.dim() == 2 or sc.shape[2] >= 1)):
        return _original_fn("sc2rk")(sc)
    dev = sc.device
    rk = torch.empty((sc.shape[0],) + tuple(sc.shape[2:]), dtype=torch.float32, device=dev)
    with _guard(dev):
        _lib.check(_entry("pings_loop_ring_key")(sc.data_ptr(), int(sc.shape[0]), int(sc.shape[1]),
                                                 int(sc.shape[2]) if sc.dim() == 3 else 0, rk.data_ptr(),
                                                 _lib.stream_ptr(dev)), "pings_loop_ring_key")
    return rk


def _read_record(record, win_tran, dev, tag):
    host = (C.c_int32 * 8)()
    _lib.check(_entry("pings_loop_read_record")(record.data_ptr(), _ptr(win_tran), C.addressof(host),
                                                _lib.stream_ptr(dev)), "pings_loop_read_record")
    _lib.note_sync(tag)
    return bytes(host)


@torch.no_grad()
def context_distance(sc1, sc2):
    """`distance_sc_torch(sc1, sc2)` for [R,S] descriptors, `distance_sc_feature_torch` for [R,S,D]: (cosine distance,
    shift in 1..S) as python numbers.  `sc1` is the one rolled.  One launch and one host read."""
    ok = (_f32_dev(sc1) and _f32_dev(sc2, sc1.device) and sc1.shape == sc2.shape and sc1.dim() in (2, 3)
          and _shape_ok(sc1.shape[0], sc1.shape[1], sc1.shape[2] if sc1.dim() == 3 else 0)
          and (sc1.dim() == 2 or sc1.shape[2] >= 1))
    if not ok:
        name = "distance_sc_feature_torch" if getattr(sc1, "dim", lambda: 2)() == 3 else "distance_sc_torch"
        return _original_fn(name)(sc1, sc2)
    dev = sc1.device
    with _guard(dev):
        record = torch.zeros(8, dtype=torch.int32, device=dev)
        _lib.check(_entry("pings_loop_context_distance")(
            sc1.data_ptr(), sc2.data_ptr(), int(sc1.shape[0]), int(sc1.shape[1]),
            int(sc1.shape[2]) if sc1.dim() == 3 else 0, record.data_ptr(), _lib.stream_ptr(dev)),
            "pings_loop_context_distance")
        raw = _read_record(record, None, dev, "loop_context_distance")
    return struct.unpack("<f", raw[12:16])[0], struct.unpack("<i", raw[16:20])[0]


# ---------------------------------------------------------------- the bank of a manager
class _Bank:
    """Descriptors of the nodes by frame id: sc [cap,R,S], rk [cap,R] and, once a node came with features,
    scf [cap,R,S,D], rkf [cap,R,D].  `stored` (host) marks the rows that hold a node."""

    def __init__(self, dev, R, S):
        self.dev, self.R, self.S, self.D, self.cap = dev, R, S, 0, 0
        self.sc = self.rk = self.scf = self.rkf = None
        self.stored = np.zeros(0, dtype=bool)
        self.stored_feat = np.zeros(0, dtype=bool)

    def ensure(self, mgr, frame_id: int, D: int) -> None:
        """Room for row `frame_id` (geometric growth, as `neural_map._ensure`); the manager's lists are rebound to the
        new rows when the arrays moved.  Device copies only."""
        grow = frame_id >= self.cap
        new_feat = D > 0 and self.scf is None
        if not (grow or new_feat):
            return
        cap = max(_BANK_MIN, 2 * self.cap, frame_id + 1) if grow else self.cap
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.dev)  # noqa: E731
        if grow:
            sc, rk = z(cap, self.R, self.S), z(cap, self.R)
            if self.cap:
                sc[:self.cap].copy_(self.sc)
                rk[:self.cap].copy_(self.rk)
            self.sc, self.rk = sc, rk
            for name in ("stored", "stored_feat"):
                a = np.zeros(cap, dtype=bool)
                a[:self.cap] = getattr(self, name)
                setattr(self, name, a)
        if D > 0 and (grow or new_feat):
            self.D = D
        if self.D > 0 and (grow or new_feat):
            scf, rkf = z(cap, self.R, self.S, self.D), z(cap, self.R, self.D)
            if self.scf is not None:
                scf[:self.cap].copy_(self.scf)
                rkf[:self.cap].copy_(self.rkf)
            self.scf, self.rkf = scf, rkf
        self.cap = cap
        for i in np.nonzero(self.stored)[0]:
            self.bind(mgr, int(i))

    def bind(self, mgr, i: int) -> None:
        mgr.contexts[i], mgr.ringkeys[i] = self.sc[i], self.rk[i]
        if self.stored_feat[i]:
            mgr.contexts_feature[i], mgr.ringkeys_feature[i] = self.scf[i], self.rkf[i]


def _bank(self, dev, create=False):
    R, S = int(self.des_shape[0]), int(self.des_shape[1])
    b = getattr(self, "_pings_bank", None)
    if b is not None and (b.dev != dev or (b.R, b.S) != (R, S)):
        b = None
    if b is None and create:
        b = self._pings_bank = _Bank(dev, R, S)
    return b


# ---------------------------------------------------------------- NeuralPointMapContextManager.add_node
def add_node(self, frame_id, ptcloud, ptfeatures=None):
    """`add_node`: the node's descriptor and ring key (M = 1, identity) written straight into the bank's row `frame_id`;
    `contexts[frame_id]` etc. are views of that row.  One library call, no host read."""
    R, S = int(self.des_shape[0]), int(self.des_shape[1])
    D = 0 if ptfeatures is None else int(ptfeatures.shape[1]) if getattr(ptfeatures, "dim", lambda: 0)() == 2 else -1
    bank = _bank(self, ptcloud.device, create=True) if _cloud_ok(ptcloud, ptfeatures) and _shape_ok(R, S) else None
    if (bank is None or not 0 <= int(frame_id) < len(self.contexts) or (D > 0 and bank.D not in (0, D))
            or getattr(self, "_pings_foreign", False)):
        self._pings_foreign = True          # a node outside the bank: this manager stays with the reference's methods
        return _original(self, "add_node")(self, frame_id, ptcloud, ptfeatures)
    i = int(frame_id)
    bank.ensure(self, i, D)
    out = (bank.sc[i:i + 1], bank.rk[i:i + 1], bank.scf[i:i + 1] if D else None, bank.rkf[i:i + 1] if D else None)
    build_contexts(ptcloud, ptfeatures, _eye12(ptcloud.device), (R, S), self.max_length, out=out)
    bank.stored[i] = True
    bank.stored_feat[i] = D > 0
    self.curr_node_idx = frame_id
    bank.bind(self, i)
    self.query_contexts = []
    self.tran_from_frame = []
    self._pings_query = None


# ---------------------------------------------------------------- NeuralPointMapContextManager.set_virtual_node
def _pose_ok(p, dev) -> bool:
    return isinstance(p, torch.Tensor) and p.device == dev and p.dtype is torch.float64 and tuple(p.shape) == (4, 4)


@torch.no_grad()
def set_virtual_node(self, ptcloud_global, frame_pose, last_frame_pose, ptfeatures=None):
    """`set_virtual_node`: the 2 * virtual_side_count + 1 lateral poses and their descriptors in two library calls and no
    host read.  The pose whose lateral offset is zero (the centre) takes the stored descriptor of `curr_node_idx`, as the
    reference does, decided on the device by the reference's own test (`norm == 0` in fp32).  `query_contexts` are views
    of one [M,R,S] / [M,R,S,D] array, `tran_from_frame` views of one [M,4,4] float64 array.  Two identical consecutive
    poses give NaN offsets, NaN transforms and therefore empty (all-zero) descriptors, as in the reference."""
    R, S = int(self.des_shape[0]), int(self.des_shape[1])
    side = int(self.virtual_side_count)
    M = 2 * side + 1
    dev = ptcloud_global.device if isinstance(ptcloud_global, torch.Tensor) else None
    bank = _bank(self, dev) if dev is not None and dev.type == "cuda" else None
    cur = int(self.curr_node_idx)
    D = 0 if ptfeatures is None else int(ptfeatures.shape[1]) if getattr(ptfeatures, "dim", lambda: 0)() == 2 else -1
    ok = (bank is not None and not getattr(self, "_pings_foreign", False) and _cloud_ok(ptcloud_global, ptfeatures)
          and _pose_ok(frame_pose, dev) and (last_frame_pose is None or _pose_ok(last_frame_pose, dev))
          and 1 <= M <= LIMITS["Q"] and 0 <= cur < bank.cap and bank.stored[cur]
          and (D == 0 or (bank.stored_feat[cur] and bank.D == D)))
    if not ok:
        self._pings_query = None
        return _original(self, "set_virtual_node")(self, ptcloud_global, frame_pose, last_frame_pose, ptfeatures)
    if not self.silence:
        print("# Augmented virtual context: ", M)
    with _guard(dev):
        transforms = torch.empty(M, 12, dtype=torch.float32, device=dev)
        tran = torch.empty(M, 4, 4, dtype=torch.float64, device=dev)
        lat = torch.empty(M, 3, dtype=torch.float32, device=dev)
        use_stored = torch.empty(M, dtype=torch.int32, device=dev)
        last = None if last_frame_pose is None else last_frame_pose.contiguous()
        _lib.check(_entry("pings_loop_virtual_poses")(
            frame_pose.contiguous().data_ptr(), _ptr(last), side, float(self.virtual_step_m), transforms.data_ptr(),
            tran.data_ptr(), lat.data_ptr(), use_stored.data_ptr(), _lib.stream_ptr(dev)), "pings_loop_virtual_poses")
    stored = (use_stored, bank.sc[cur], bank.rk[cur], bank.scf[cur] if D else None, bank.rkf[cur] if D else None)
    sc, rk, scf, rkf = build_contexts(ptcloud_global, ptfeatures, transforms, (R, S), self.max_length, stored=stored)
    ctx = sc if D == 0 else scf
    new_q, new_t = [ctx[k] for k in range(M)], [tran[k] for k in range(M)]
    # the reference appends: after add_node (which clears both lists) that is the same as assigning
    self.query_contexts.extend(new_q)
    self.tran_from_frame.extend(new_t)
    fresh = len(self.query_contexts) == M
    self._pings_query = {"list": self.query_contexts, "M": M, "feature": D > 0, "ctx": ctx, "key": rk if D == 0 else rkf,
                         "lat": lat} if fresh else None


# ---------------------------------------------------------------- NeuralPointMapContextManager.detect_loop
def _cand_dev(cand: np.ndarray, dev) -> torch.Tensor:
    """int32 slots on the device through pinned memory: an asynchronous copy, no host wait."""
    host = torch.from_numpy(np.ascontiguousarray(cand, dtype=np.int32)).pin_memory()
    return host.to(dev, non_blocking=True)


@torch.no_grad()
def detect_loop(self, candidate_idx, use_feature: bool = False):
    """`detect_loop`: (loop_id, cosine distance, 4x4 numpy T_l<-c) or (None, None, None).  Two launches and one host
    read; the yaw matrix and the product with the winning query's `tran_from_frame` are host arithmetic on the record
    (the winner's lateral offset travels in it: its entries are float32 values, so the float64 matrix is exact)."""
    cand = np.asarray(candidate_idx)
    if cand.shape[0] == 0:
        return None, None, None
    bank = getattr(self, "_pings_bank", None)
    use_feature = bool(use_feature)
    q = getattr(self, "_pings_query", None)
    n_q = len(self.query_contexts)
    ok = (bank is not None and not getattr(self, "_pings_foreign", False) and cand.ndim == 1
          and cand.dtype.kind in "iu" and cand.shape[0] <= LIMITS["C"] and int(cand.min()) >= 0
          and int(cand.max()) < bank.cap and (not use_feature or bank.scf is not None)
          and bool((bank.stored_feat if use_feature else bank.stored)[cand].all()))
    if ok and n_q:
        ok = q is not None and q["list"] is self.query_contexts and n_q == q["M"] and q["feature"] == use_feature
    cur = int(self.curr_node_idx)
    if ok and not n_q:
        ok = 0 <= cur < bank.cap and bool((bank.stored_feat if use_feature else bank.stored)[cur])
    if not ok:
        return _original(self, "detect_loop")(self, candidate_idx, use_feature)
    dev = bank.dev
    R, S, D = bank.R, bank.S, bank.D
    b_ctx, b_key = (bank.scf, bank.rkf) if use_feature else (bank.sc, bank.rk)
    with _guard(dev):
        if n_q == 0:                         # :241-248: the current node is the one query
            self.tran_from_frame.append(torch.eye(4, device=dev, dtype=torch.float64))
            self.query_contexts.append((self.contexts_feature if use_feature else self.contexts)[cur])
            q_ctx, q_key, lat, Q = b_ctx[cur], b_key[cur], None, 1
        else:
            q_ctx, q_key, lat, Q = q["ctx"], q["key"], q["lat"], q["M"]
        record = torch.zeros(8, dtype=torch.int32, device=dev)
        win = torch.zeros(3, dtype=torch.float32, device=dev)
        cand_dev = _cand_dev(cand, dev)
        _lib.check(_entry("pings_loop_search")(
            b_ctx.data_ptr(), b_key.data_ptr(), bank.cap, cand_dev.data_ptr(), int(cand.shape[0]), q_ctx.data_ptr(),
            q_key.data_ptr(), Q, R, S, D, int(use_feature), float(self.ringkey_dist_thre), _ptr(lat),
            record.data_ptr(), win.data_ptr(), _lib.stream_ptr(dev)), "pings_loop_search")
        raw = _read_record(record, win, dev, "loop_detect")
    cpos, _, rk_dist, cosdist, shift, tx, ty, tz = struct.unpack("<iiffifff", raw)
    if not self.silence:
        print("min ringkey dist:", rk_dist)
    if cpos < 0 or rk_dist > self.ringkey_dist_thre:
        return None, None, None
    if not self.silence:
        print("min context cos dist:", cosdist)
    if not cosdist < self.sc_cosdist_threshold:
        return None, None, None
    yawdiff_deg = shift * (360.0 / self.des_shape[1])
    if not self.silence:
        print("yaw diff deg:", yawdiff_deg)
    yawdiff_rad = math.radians(yawdiff_deg)
    cos_yaw, sin_yaw = math.cos(yawdiff_rad), math.sin(yawdiff_rad)
    transformation = np.eye(4)
    transformation[0, 0], transformation[0, 1] = cos_yaw, sin_yaw
    transformation[1, 0], transformation[1, 1] = -sin_yaw, cos_yaw          # T_l<-c'
    from_frame = np.eye(4)
    from_frame[:3, 3] = (tx, ty, tz)                                        # zeros without virtual nodes
    return int(cand[cpos]), cosdist, transformation @ from_frame            # T_l<-c = T_l<-c' @ T_c'<-c


# ---------------------------------------------------------------- install
_METHODS = (("add_node", add_node), ("set_virtual_node", set_virtual_node), ("detect_loop", detect_loop))


def install(loop_detector_module) -> None:
    """`import utils.loop_detector as ld; install(ld)`: rebinds `ptcloud2sc_torch`, `sc2rk`, `distance_sc_torch`,
    `distance_sc_feature_torch` of the module and `add_node`, `set_virtual_node`, `detect_loop` of its
    `NeuralPointMapContextManager`.  The originals are kept for the fallbacks and for `uninstall`.  Installing twice
    changes nothing."""
    from .pool_ops import _rebind

    g = globals()
    for ref_name, own in _FUNCTIONS:
        cur = getattr(loop_detector_module, ref_name)
        if cur is not g[own]:
            _originals[ref_name] = cur
            setattr(loop_detector_module, ref_name, g[own])
    for name, fn in _METHODS:
        _rebind(loop_detector_module.NeuralPointMapContextManager, name, fn)


def uninstall(loop_detector_module) -> None:
    """Puts the reference's own functions and methods back wherever `install` replaced them."""
    from .pool_ops import _restore

    g = globals()
    for ref_name, own in _FUNCTIONS:
        if getattr(loop_detector_module, ref_name, None) is g[own] and ref_name in _originals:
            setattr(loop_detector_module, ref_name, _originals.pop(ref_name))
    for name, fn in _METHODS:
        _restore(loop_detector_module.NeuralPointMapContextManager, name, fn)
