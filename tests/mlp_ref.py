"""Helpers of tests/test_mlp_plan_edges.py: the decoder MLP in plain fp64 with per-element fp32 error bounds, a Python
restatement of `mlp_plan` (csrc/mlp_common.hpp), and the kernel classes read out of the three kernel files.

Reference.  `y = relu(x W1^T + b1) W2^T + b2` and its five gradients, written out as matrix products (no autograd), and
the double backward of `mlp_h64o1.hip`'s header comment.  Next to every output stands E, a bound on |fp32 result - fp64
result| per element that holds for ANY order of an fp32 sum of products (MFMA fma chains, fixed-order LDS sums, the
eight-chain reduce kernel): with u = 2^-24 and gamma(n) = n u / (1 - n u), a sum of n products of fp32 numbers is off
by at most gamma(n) * (sum of the products' absolute values) (Higham, Accuracy and Stability of Numerical Algorithms,
section 3.1: every term passes through at most one multiplication and n - 1 additions), and an operand that itself
carries an error e adds |other operand| * e to first order.  With m = [pre > 0]:

    E_pre = gamma(IN + 1) (|x| |W1|^T + |b1|)            E_h = E_pre * m
    E_y   = gamma(HID + 1) (h |W2|^T + |b2|) + E_h |W2|^T
    E_gh  = gamma(OUT) (|gy| |W2|) * m
    E_gx  = gamma(HID) |gh| |W1| + E_gh |W1|
    E_gW1 = gamma(N) |gh|^T |x| + E_gh^T |x|             E_gb1 = gamma(N) sum |gh| + sum E_gh
    E_gW2 = gamma(N) |gy|^T h + |gy|^T E_h               E_gb2 = gamma(N) sum |gy|

and for the double backward (a = dL/dgx, u = a W1^T, gH2 = gy m W2, one product each):

    E_u   = gamma(IN) |a| |W1|^T
    E_ggy = gamma(HID) (m |u|) |W2|^T + (m E_u) |W2|^T
    E_gW2 = gamma(N) sum_n |gy| m |u| + sum_n |gy| m E_u
    E_gW1 = gamma(N) |gH2|^T |a| + (gamma(1) |gH2|)^T |a|

Every bound gets an absolute floor of n 2^-126 (n = terms of the sum) for products flushed to zero.  Zero padding adds
exact zeros and so nothing to any bound.  The bounds assume the fp32 mask equals the fp64 one, which `nudge_off_kink`
guarantees: no pre-activation is left within 2 E_pre of zero.  That is also why E_h carries the mask: where pre < 0 by
more than its own error, both the fp32 and the fp64 h are exactly zero, so a masked unit brings no error into y or gW2.
"""
from __future__ import annotations

import re
from collections import namedtuple
from pathlib import Path

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
CSRC = Path(__file__).resolve().parent.parent / "pings_amd" / "csrc"


def gamma(n):
    return n * U / (1.0 - n * U)


def _d(t):
    return t.detach().double().cpu()


def pre_bound(x, W1, b1):
    """fp64 pre-activation [N, HID] and E_pre."""
    x, W1, b1 = _d(x), _d(W1), _d(b1)
    IN = x.shape[1]
    pre = x @ W1.T + b1
    return pre, gamma(IN + 1) * (x.abs() @ W1.abs().T + b1.abs()) + (IN + 1) * TINY


def nudge_off_kink(x, W1, b1, rounds=8):
    """Moves (in place, by +0.01) the rows of x with a pre-activation within 2 E_pre of the ReLU kink, where fp32 and
    fp64 may disagree about the mask and no gradient is defined.  Returns how many rows were moved."""
    moved = torch.zeros(x.shape[0], dtype=torch.bool)
    for rnd in range(rounds + 1):
        pre, E = pre_bound(x, W1, b1)
        kink = (pre.abs() <= 2.0 * E).any(dim=1)
        if not kink.any():
            break
        assert rnd < rounds, f"{int(kink.sum())} rows still on the ReLU kink after {rounds} nudges"
        x[kink] += 0.01
        moved |= kink
    return int(moved.sum())


def draw_inputs(N, IN, HID, OUT, seed):
    """fp32 CPU tensors (x, W1, b1, W2, b2, gy) in the distributions of test_mlp.py (randn, W / sqrt(fan_in), 0.2 randn
    biases) with x nudged off the kink, and how many rows the nudge moved."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, IN, generator=g)
    W1, b1 = torch.randn(HID, IN, generator=g) / IN ** 0.5, 0.2 * torch.randn(HID, generator=g)
    W2, b2 = torch.randn(OUT, HID, generator=g) / HID ** 0.5, 0.2 * torch.randn(OUT, generator=g)
    gy = torch.randn(N, OUT, generator=g)
    return (x, W1, b1, W2, b2, gy), nudge_off_kink(x, W1, b1)


def make_inputs(N, IN, HID, OUT, seed):
    """`draw_inputs` with the gate on the rows moved.  From 300 rows on, fewer than 1 % of the rows may have been moved.
    Below 300 rows one row is already more than 1 %, so there a case may move at most three rows, and
    test_mlp_plan_edges.py holds the fraction over all of its small cases together below 1 %."""
    ins, moved = draw_inputs(N, IN, HID, OUT, seed)
    check_moved(moved, N)
    return ins


def check_moved(moved, N):
    """The gate on the rows `nudge_off_kink` moved (see make_inputs)."""
    if N >= 300:
        assert moved < 0.01 * N, f"{moved} of {N} rows were moved off the kink"
    else:
        assert moved <= 3, f"{moved} of {N} rows were moved off the kink"


def first_order(x, W1, b1, W2, b2, gy):
    """{name: (fp64 value, E)} for y, gx, gW1, gb1, gW2, gb2."""
    x, W1, b1, W2, b2, gy = (_d(t) for t in (x, W1, b1, W2, b2, gy))
    N, IN = x.shape
    HID, OUT = W1.shape[0], W2.shape[0]
    pre, E_pre = pre_bound(x, W1, b1)
    m = (pre > 0).double()
    h = pre * m
    E_h = E_pre * m
    aW1, aW2, ax, agy = W1.abs(), W2.abs(), x.abs(), gy.abs()
    out = {}
    out["y"] = (h @ W2.T + b2, gamma(HID + 1) * (h @ aW2.T + b2.abs()) + E_h @ aW2.T + (HID + 1) * TINY)
    gh = (gy @ W2) * m
    agh = gh.abs()
    E_gh = (gamma(OUT) * (agy @ aW2) + OUT * TINY) * m
    out["gx"] = (gh @ W1, gamma(HID) * (agh @ aW1) + E_gh @ aW1 + HID * TINY)
    out["gW1"] = (gh.T @ x, gamma(N) * (agh.T @ ax) + E_gh.T @ ax + N * TINY)
    out["gb1"] = (gh.sum(0), gamma(N) * agh.sum(0) + E_gh.sum(0) + N * TINY)
    out["gW2"] = (gy.T @ h, gamma(N) * (agy.T @ h) + agy.T @ E_h + N * TINY)
    out["gb2"] = (gy.sum(0), gamma(N) * agy.sum(0) + N * TINY)
    return out


def double_backward(x, a, gy, W1, b1, W2):
    """{name: (fp64 value, E)} for ggy [N, 1], gW1, gW2 [1, HID] of the backward of gx = gy (m * W2) W1 (OUT = 1)
    under the cotangent a [N, IN]."""
    x, a, gy, W1, b1, W2 = (_d(t) for t in (x, a, gy, W1, b1, W2))
    N, IN = x.shape
    HID = W1.shape[0]
    assert W2.shape == (1, HID)
    g = gy.reshape(N, 1)
    pre, _ = pre_bound(x, W1, b1)
    m = (pre > 0).double()
    aa, aW2 = a.abs(), W2.abs()
    u = a @ W1.T
    au = m * u.abs()
    E_u = m * (gamma(IN) * (aa @ W1.abs().T) + IN * TINY)
    out = {}
    out["ggy"] = ((m * u) @ W2.T, gamma(HID) * (au @ aW2.T) + E_u @ aW2.T + HID * TINY)
    out["gW2"] = ((g * m * u).sum(0, keepdim=True),
                  (gamma(N) * (g.abs() * au).sum(0) + (g.abs() * E_u).sum(0) + N * TINY).reshape(1, HID))
    gH2 = g * m * W2
    E_gH2 = gamma(1) * gH2.abs() + TINY
    out["gW1"] = (gH2.T @ a, gamma(N) * (gH2.abs().T @ aa) + E_gH2.T @ aa + N * TINY)
    return out


def worst_ratio(got, ref, E):
    """max |got - ref| / E over the elements (E > 0 everywhere: the floor)."""
    got = _d(got).reshape(ref.shape)
    assert torch.isfinite(got).all()
    return float(((got - ref).abs() / E).max()) if ref.numel() else 0.0


# ---------------------------------------------------------------- the plan, restated
# family names; the numbers are the template arguments of the kernels (csrc/mlp_common.hpp: Plan)
Sig = namedtuple("Sig", "hid fwd bwd fwd_ks h64 fwd_pfx bwd_pf wave wave_store")


OPERANDS = ("x", "gy", "W1", "W2")      # the operands whose alignment the wave-128 kernels look at


def plan(IN, HID, OUT, misaligned=()):
    """Class signature of the kernels that shape (IN, HID, OUT) runs.  `misaligned` names the operands among OPERANDS
    that do not start on a 16-byte boundary.  Fields a family does not use are None."""
    def al(name):
        return name not in misaligned

    wave128, h64o1 = HID == 128 and IN <= 32, HID == 64 and OUT == 1
    bwd = "wave128" if wave128 else "h64o1" if h64o1 else "wg"
    fwd = "wg" if (h64o1 and IN > 35) else bwd
    fwd_ks = h64 = fwd_pfx = bwd_pf = wave = wave_store = None
    if fwd == "h64o1":      # 2 KS registers hold the row and the bias column
        fwd_ks = 6 if IN <= 11 else 10 if IN <= 19 else 18
    if bwd == "h64o1":      # two inputs per k-step, a second 32-wide block of inputs beyond 32
        h64 = (6, 1) if IN <= 12 else (16, 1) if IN <= 32 else (18, 2) if IN <= 36 else (32, 2)
    inp = IN + (IN & 1)
    nthr = 2 * HID
    need = -(-32 * inp // nthr)     # registers per thread that hold a 32-row tile of x
    if fwd == "wg":
        fwd_pfx = next(c for c in (5, 10, 18, 32) if need <= c)
    if bwd == "wg":
        classes = {128: (5, 9), 96: (6, 11), 64: (9, 16), 32: (18, 32)}[HID]
        bwd_pf = (next(c for c in classes if need <= c), {128: 4, 96: 6, 64: 8, 32: 16}[HID])
    if wave128:
        vecg = OUT % 4 == 0 and al("gy")
        oh = 16 if not vecg else 12 if OUT == 24 else 4 if OUT == 8 else 16
        wave = (IN % 4 == 0 and al("W1") and al("W2"), IN % 4 == 0 and al("x"), oh, vecg)
        wave_store = OUT % 4 == 0
    return Sig(HID, fwd, bwd, fwd_ks, h64, fwd_pfx, bwd_pf, wave, wave_store)


def admitted_shapes():
    """Every (IN, HID, OUT) check_dims (csrc/mlp.hip) admits."""
    return [(IN, HID, OUT) for HID in (32, 64, 96, 128) for IN in range(1, 65) for OUT in range(1, 33)]


def reachable_signatures():
    """{signature: (smallest IN, largest IN)} over all admitted shapes with aligned operands."""
    span = {}
    for IN, HID, OUT in admitted_shapes():
        s = plan(IN, HID, OUT)
        lo, hi = span.get(s, (IN, IN))
        span[s] = (min(lo, IN), max(hi, IN))
    return span


def reachable_classes():
    """The kernel template classes the restated plan can ask for, keyed as `built_classes` keys them."""
    out = {"wg_fwd": set(), "wg_bwd": set(), "h64o1_fwd": set(), "h64o1_bwd": set(), "wave128_bwd": set()}
    for IN, HID, OUT in admitted_shapes():
        for mis in ((), OPERANDS):
            s = plan(IN, HID, OUT, mis)
            if s.fwd_pfx is not None:
                out["wg_fwd"].add(s.fwd_pfx)
            if s.bwd_pf is not None:
                out["wg_bwd"].add(s.bwd_pf)
            if s.fwd_ks is not None:
                out["h64o1_fwd"].add(s.fwd_ks)
            if s.h64 is not None:
                out["h64o1_bwd"].add(s.h64)     # backward and double backward share with_h64o1_class
            if s.wave is not None:
                out["wave128_bwd"].add((s.wave[2], s.wave[1], s.wave[3]))
    return out


_WITH_CLASS = re.compile(r"with_class<([\d,\s]+)>\(p\.(\w+)")
_SECOND = re.compile(r"integral_constant<int,\s*(\d+)>\{\}")
_BODY = re.compile(r"PINGS_BWD_BODY\((\d+),\s*VX_,\s*(true|false)\)")
_VX = re.compile(r"PINGS_BWD_CLASS\((true|false)\);")


def built_classes(csrc=CSRC):
    """The classes the kernel files instantiate: the `with_class<...>` lists of mlp_wg.hip and mlp_h64o1.hip and the
    `PINGS_BWD_BODY(...)` lines of mlp_wave128.hip."""
    lists = {}
    for name in ("mlp_wg.hip", "mlp_h64o1.hip"):
        for line in (csrc / name).read_text().splitlines():
            mc = _WITH_CLASS.search(line)
            if not mc:
                continue
            vals = [int(v) for v in mc.group(1).split(",")]
            second = _SECOND.search(line)
            lists.setdefault(mc.group(2), set()).update((v, int(second.group(1))) if second else v for v in vals)
    wave = (csrc / "mlp_wave128.hip").read_text()
    bodies = {(int(oh), vg == "true") for oh, vg in _BODY.findall(wave)}
    vxs = {v == "true" for v in _VX.findall(wave)}
    return {"wg_fwd": lists.get("fwd_pfx", set()), "wg_bwd": lists.get("bwd_pfx", set()),
            "h64o1_fwd": lists.get("fwd_ks", set()), "h64o1_bwd": lists.get("h64_ns", set()),
            "wave128_bwd": {(oh, vx, vg) for oh, vg in bodies for vx in vxs}}


_WITH_CLASS_WHAT = re.compile(r'with_class<([\d,\s]+)>\(\s*[\w.]+,\s*"([^"]+)"')


def with_class_lists(*names, csrc=CSRC):
    """{what: classes} of every `with_class<...>(v, "what", ...)` call in the named kernel files, keyed by the string
    the call names itself with (the fused SDF query's four launches; the decoder MLP's all say "decoder MLP")."""
    out = {}
    for name in names:
        for vals, what in _WITH_CLASS_WHAT.findall((csrc / name).read_text()):
            out.setdefault(what, set()).update(int(v) for v in vals.split(","))
    return out
