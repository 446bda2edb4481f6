"""The colour and semantic heads (pings_amd/csrc/heads.hip) through `pings_head_reduce` and `mesher_ops.head_reduce`
against fp64 torch, at the launch edges of B, k and C, with logits that overflow `expf`, with offsets that need the
max-subtraction of the log-softmax, on ties of the arg-max, and past the 16 neighbours the semantic kernel holds in
registers.

    colour    out[b, c]  = sum_j w_j sigmoid(raw[b, j, c])
    semantic  prob[b, c] = sum_j w_j log_softmax(raw[b, j, :])[c],  label[b] = argmax_c prob[b, c] (first maximum)

Bounds, u = 2^-24.  Colour: the sigmoid of one neighbour carries the rounding of 1 + e, of the division and of the
product with w_j (3 u) and passes at most k - 1 additions, so (k + 4) u sum_j |w_j| with one spare; on top the relative
error of `expf`, for which the golden test of the heads (tests/test_mesher.py) allows 1e-5 of sum_j w_j = 1.  Semantic:
raw - max, the sum of exponentials, its logarithm, max + log, raw - lse, the product and the additions over j are each
rounded at a magnitude of at most |raw|_max + log C, so 8 u sum_j |w_j| (|raw|_max + log C).  A label is compared
wherever the two best fp64 sums are further apart than twice that bound.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

U = 2.0 ** -24
EXPF_REL = 1e-5            # what tests/test_mesher.py allows the colour head on weights that sum to one
MID = dict(B=257, k=4, C=4)
B_EDGES, K_EDGES, C_EDGES = (0, 1, 255, 256, 257, 65537), (1, 2, 15, 16), (1, 3, 4, 20, 33)
# edge values of each axis with mid values of the others; "w": weights given, "none": NULL (weight one)
SHAPES = sorted({(B, MID["k"], MID["C"], "w") for B in B_EDGES} | {(MID["B"], k, MID["C"], "w") for k in K_EDGES} |
                {(MID["B"], MID["k"], Cn, "w") for Cn in C_EDGES} | {(MID["B"], 1, MID["C"], "none"),
                                                                    (MID["B"], MID["k"], MID["C"], "none")})
BIG_K = (17, 24, 64)


def _weights(rng, B, k, mode):
    if mode == "none":
        return None
    w = rng.uniform(0.05, 1.0, (B, k))
    w /= w.sum(1, keepdims=True)             # IDW weights sum to one ...
    w[1::7] *= 1.7                           # ... but nothing in the kernel may depend on it
    return w.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _colour_case(B, k, Cn, mode):
    """raw, w (fp32 numpy), fp64 reference and its bound.  The first rows hold the logits at which `expf` overflows."""
    rng = np.random.default_rng(B * 131 + k * 17 + Cn)
    raw = rng.normal(0.0, 3.0, (B, k, Cn)).astype(np.float32)
    special = (100.0, -100.0, 88.8, -88.8)
    for i, v in enumerate(special[:B]):
        raw[i] = v                           # every neighbour, every channel: the result is sum_j w_j or 0
    if B > len(special):
        raw[len(special), :, 0] = special[:1] * k
        raw[len(special), 0, :] = -88.8      # mixed with ordinary logits in one row
    w = _weights(rng, B, k, mode)
    w64 = torch.ones(B, k, dtype=torch.float64) if w is None else torch.from_numpy(w).double()
    ref = (w64.unsqueeze(-1) * torch.sigmoid(torch.from_numpy(raw).double())).sum(1)
    bound = ((k + 4) * U + EXPF_REL) * w64.abs().sum(1, keepdim=True).expand(B, Cn)
    return raw, w, ref.numpy(), bound.numpy(), ((k + 4) * U * w64.abs().sum(1, keepdim=True).expand(B, Cn)).numpy()


@functools.lru_cache(maxsize=None)
def _sem_case(B, k, Cn, mode, tie_pair=None):
    """raw, w, fp64 prob, label, bound[B], rows whose label is decided (top-two gap > 2 bound), tie rows."""
    rng = np.random.default_rng(B * 137 + k * 19 + Cn)
    raw = rng.normal(0.0, 3.0, (B, k, Cn))
    # offsets per neighbour: the log-softmax does not see them, `expf` without the max-subtraction does
    off = np.zeros((B, k, 1))
    off[0::5], off[1::5] = 80.0, -80.0
    off[2::20] = 1e4
    off[3::20, ::2] = 1e4                    # only every other neighbour of a row
    raw = (raw + off).astype(np.float32)
    ties = np.zeros(B, bool)
    if tie_pair is not None:
        lo, hi = tie_pair
        ties[4::3] = True
        top = raw.max(2) + 1.0               # the two tied classes carry the largest logit of every neighbour
        raw[ties, :, lo] = top[ties]
        raw[ties, :, hi] = top[ties]
    w = _weights(rng, B, k, mode)
    w64 = torch.ones(B, k, dtype=torch.float64) if w is None else torch.from_numpy(w).double()
    r64 = torch.from_numpy(raw).double()
    prob = (w64.unsqueeze(-1) * torch.log_softmax(r64, dim=-1)).sum(1)
    label = torch.argmax(prob, dim=1)
    bound = 8 * U * w64.abs().sum(1) * (r64.abs().amax((1, 2)) + np.log(Cn)) if B else torch.zeros(0, dtype=torch.float64)
    if Cn > 1:
        top2 = torch.topk(prob, 2, dim=1).values
        decided = (top2[:, 0] - top2[:, 1]) > 2 * bound
    else:
        decided = torch.ones(B, dtype=torch.bool)
    return raw, w, prob.numpy(), label.numpy(), bound.numpy(), decided.numpy(), ties


def test_reference_decides_all_but_one_percent_of_the_labels():
    """The inputs of the label comparisons: at most 1 % of the rows have their two best classes within twice the bound."""
    for B, k, Cn, mode in SHAPES:
        if B >= 255:
            _, _, _, _, _, decided, _ = _sem_case(B, k, Cn, mode)
            assert decided.mean() >= 0.99, (B, k, Cn, mode, decided.mean())
    for k in (17, 24):
        assert _sem_case(MID["B"], k, MID["C"], "w")[5].mean() >= 0.99


# ================================================================ device
def _reduce(raw, w, B, k, Cn, mode, want_value=True, want_label=True):
    """`pings_head_reduce` on buffers of full size: (status, value[B, C] | None, label[B] | None)."""
    from pings_amd import _lib

    L = _lib.lib()
    up = lambda a, shape: torch.zeros(max(int(np.prod(shape)), 1), dtype=torch.float32, device="cuda") if a is None else \
        torch.cat([torch.from_numpy(np.ascontiguousarray(a)).reshape(-1), torch.zeros(1)]).cuda()
    d_raw = up(raw, (B, k, Cn))
    d_w = None if w is None else up(w, (B, k))
    val = torch.full((max(B * Cn, 1),), -7.0, device="cuda") if want_value else None
    lab = torch.full((max(B, 1),), -7, dtype=torch.int64, device="cuda") if want_label else None
    rc = L.pings_head_reduce(d_raw.data_ptr(), None if d_w is None else d_w.data_ptr(), B, k, Cn, mode,
                             None if val is None else val.data_ptr(), None if lab is None else lab.data_ptr(),
                             _lib.stream_ptr(torch.device("cuda", torch.cuda.current_device())))
    torch.cuda.synchronize()
    return rc, None if val is None else val.cpu().numpy()[:B * Cn].reshape(B, Cn), \
        None if lab is None else lab.cpu().numpy()[:B]


def _check_colour(got, ref, bound, tight, tag):
    assert not np.isnan(got).any()
    err = np.abs(got.astype(np.float64) - ref)
    r = float((err / bound).max()) if err.size else 0.0
    r_tight = float((err / tight).max()) if err.size else 0.0
    print(f"\n[colour {tag}] error / bound {r:.3g}  (error / the rounding part of the bound alone {r_tight:.3g})")
    assert r <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("B,k,Cn,mode", SHAPES)
def test_colour_head_matches_fp64(B, k, Cn, mode):
    from pings_amd import _abi, mesher_ops as MO

    raw, w, ref, bound, tight = _colour_case(B, k, Cn, mode)
    rc, got, _ = _reduce(raw, w, B, k, Cn, _abi.HEAD_COLOR, want_label=False)
    assert rc == 0
    _check_colour(got, ref, bound, tight, f"B={B} k={k} C={Cn} {mode}")
    if B >= 4 and w is None and k == 1:      # expf overflows to Inf at 100 and 88.8: exactly 1, 0, 1, 0, never NaN
        assert np.all(got[0] == 1.0) and np.all(got[1] == 0.0) and np.all(got[2] == 1.0) and np.all(got[3] == 0.0)
    # the wrapper: [B, k, C] with weights [B, k, 1], or [B, C] for k = 1 without weights; the same kernel, the same bits
    t_raw = torch.from_numpy(raw).cuda()
    if w is None and k == 1:
        out = MO.head_reduce(t_raw.reshape(B, Cn), None, _abi.HEAD_COLOR)
    else:
        out = MO.head_reduce(t_raw, None if w is None else torch.from_numpy(w).cuda().reshape(B, k, 1), _abi.HEAD_COLOR)
    assert out.shape == (B, Cn) and np.array_equal(out.cpu().numpy().view(np.int32), got.view(np.int32))


def _check_sem(prob, label, case, tag):
    raw, w, ref, ref_label, bound, decided, ties = case
    if prob is not None:
        assert not np.isnan(prob).any()
        err = np.abs(prob.astype(np.float64) - ref).max(1) if prob.size else np.zeros(0)
        with np.errstate(invalid="ignore"):
            ok = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
        r = float(ok.max()) if ok.size else 0.0
        print(f"\n[semantic {tag}] prob error / bound {r:.3g}  labels compared {decided.mean() if decided.size else 1:.4f}")
        assert r <= 1.0
    check = decided & ~ties
    assert np.array_equal(label[check], ref_label[check])
    assert label.size == 0 or (label.min() >= 0 and label.max() < raw.shape[2])


@pytest.mark.gpu
@pytest.mark.parametrize("B,k,Cn,mode", SHAPES)
def test_semantic_head_matches_fp64(B, k, Cn, mode):
    from pings_amd import _abi, mesher_ops as MO

    case = _sem_case(B, k, Cn, mode)
    raw, w = case[0], case[1]
    rc, prob, label = _reduce(raw, w, B, k, Cn, _abi.HEAD_SEMANTIC)
    assert rc == 0
    _check_sem(prob, label, case, f"B={B} k={k} C={Cn} {mode}")
    if Cn == 1:                              # log_softmax of one class: raw - (max + log 1) = 0 exactly
        assert np.all(prob == 0.0) and np.all(label == 0)
    rc, _, label2 = _reduce(raw, w, B, k, Cn, _abi.HEAD_SEMANTIC, want_value=False)      # out_value == NULL
    assert rc == 0 and np.array_equal(label, label2)
    t_raw = torch.from_numpy(raw).cuda()
    if w is None and k == 1:
        out = MO.head_reduce(t_raw.reshape(B, Cn), None, _abi.HEAD_SEMANTIC)
    else:
        out = MO.head_reduce(t_raw, None if w is None else torch.from_numpy(w).cuda().reshape(B, k, 1), _abi.HEAD_SEMANTIC)
    assert out.dtype == torch.int64 and np.array_equal(out.cpu().numpy(), label)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [(0, 3), (1, 2), (2, 19)])
def test_semantic_arg_max_takes_the_first_of_two_equal_classes(pair):
    """Two classes with bit-identical columns in every neighbour have bit-identical sums; where they are the largest,
    torch.argmax returns the lower index.  Pairs at the first class, in the middle and at the last class."""
    from pings_amd import _abi

    B, k, Cn = MID["B"], MID["k"], 20 if pair[1] > 3 else 4
    case = _sem_case(B, k, Cn, "w", pair)
    rc, prob, label = _reduce(case[0], case[1], B, k, Cn, _abi.HEAD_SEMANTIC)
    ties = case[6]
    assert rc == 0 and ties.sum() > 50
    assert np.array_equal(prob[ties][:, pair[0]].view(np.int32), prob[ties][:, pair[1]].view(np.int32))
    assert np.all(prob[ties].argmax(1) == pair[0])          # the two are the largest on the device as well
    assert np.all(label[ties] == pair[0])
    _check_sem(prob, label, case, f"ties {pair}")


@pytest.mark.gpu
@pytest.mark.parametrize("k", BIG_K)
def test_colour_head_has_no_limit_on_k(k):
    from pings_amd import _abi, mesher_ops as MO

    B, Cn = MID["B"], 3
    raw, w, ref, bound, tight = _colour_case(B, k, Cn, "w")
    rc, got, _ = _reduce(raw, w, B, k, Cn, _abi.HEAD_COLOR, want_label=False)
    assert rc == 0
    _check_colour(got, ref, bound, tight, f"B={B} k={k} C={Cn}")
    out = MO.head_reduce(torch.from_numpy(raw).cuda(), torch.from_numpy(w).cuda().reshape(B, k, 1), _abi.HEAD_COLOR)
    assert np.array_equal(out.cpu().numpy().view(np.int32), got.view(np.int32))


@pytest.mark.gpu
def test_entry_refuses_what_it_cannot_do():
    """PINGS_ERR_ARG (1) and nothing written: k = 0, C = 0, an unknown mode, and the semantic mode past 16 neighbours."""
    from pings_amd import _abi

    B, Cn = 8, 4
    raw = np.zeros((B, 17, Cn), np.float32)
    for k, c, mode in ((0, Cn, _abi.HEAD_COLOR), (4, 0, _abi.HEAD_COLOR), (4, Cn, 2), (4, Cn, -1),
                       (17, Cn, _abi.HEAD_SEMANTIC), (0, Cn, _abi.HEAD_SEMANTIC)):
        rc, val, lab = _reduce(raw, None, B, k, c, mode)
        assert rc == 1, (k, c, mode)
        assert np.all(val == -7.0) and np.all(lab == -7)
    assert _reduce(raw[:, :16], None, B, 16, Cn, _abi.HEAD_SEMANTIC)[0] == 0
    assert _reduce(raw, None, B, 17, Cn, _abi.HEAD_COLOR)[0] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("k", (17, 24))
def test_wrapper_labels_past_sixteen_neighbours(k):
    """`mesher_ops.head_reduce` composes the reference's log_softmax, weighted sum and argmax for k > 16 (a config with a
    larger query_nn_k).  Checked at the wrapper alone: a `Mesher` / `Tracker` query cannot be made with more than 16
    neighbours, the kNN search in front of the heads refuses it (`nn_k must be in 1..16`, csrc/knn_host.hpp)."""
    from pings_amd import _abi, mesher_ops as MO

    B, Cn = MID["B"], MID["C"]
    case = _sem_case(B, k, Cn, "w")
    out = MO.head_reduce(torch.from_numpy(case[0]).cuda(), torch.from_numpy(case[1]).cuda().reshape(B, k, 1),
                         _abi.HEAD_SEMANTIC)
    assert out.dtype == torch.int64 and out.shape == (B,)
    _check_sem(None, out.cpu().numpy(), case, f"k={k}")
    none = _sem_case(B, k, Cn, "none")
    out = MO.head_reduce(torch.from_numpy(none[0]).cuda(), None, _abi.HEAD_SEMANTIC)
    _check_sem(None, out.cpu().numpy(), none, f"k={k} none")
