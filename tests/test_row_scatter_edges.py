"""Deterministic row scatter-add (csrc/row_scatter.hip: the backward of the feature-table gathers) at its edges.

`pings_rows_scatter_add` sorts the pairs by destination row (histogram, scan, placement, rank) and sums every row in
ascending pair id with one of two kernels: `gather_sum_kernel` walks the table (one lane group per ROW) and
`gather_bucket_kernel` walks the sorted pairs (one lane group per PAIR, the first pair of a bucket works; the table is
zeroed first).  The host takes the bucket kernel when `4 * n_pairs < rows`.  The reference is an fp64 `index_add_` on
the CPU.

Most cases are made exact: `src` holds integers |v| <= 64, `w` is drawn from {0.5, 1, 2} and a row receives at most
256 pairs, so every product is a multiple of 0.5 of magnitude <= 128 and every partial sum a multiple of 0.5 below
2^15 — exact in fp32 in any order of additions, fused or not.  The result must then EQUAL the fp64 reference: one
missing, duplicated or misrouted pair cannot hide behind a tolerance.  One random-valued case per kernel path keeps the
project's bound `rel_err <= 1e-5` (tests/test_sdf.py, `test_rows_scatter_add_is_exact_and_reproducible`)."""
import pytest
import torch

from conftest import rel_err

F_ALL = [1, 2, 3, 4, 5, 8, 12, 13, 20, 33, 61, 64]     # lane classes G = 1, 2, 4, 8, 16; idle lanes at 12, 20, 33
PATHS = ["table", "bucket"]


def _rows_for(path, n):
    """Row count on either side of the host's switch `4 * n_pairs < rows`."""
    return 4 * n if path == "table" else 4 * n + 1


def _takes_bucket_kernel(n, rows):
    return 4 * n < rows                                 # row_scatter.hip: gather_sum()


def _exact_inputs(seed, n, n_src, ld):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(-64, 65, (n_src, ld), generator=g).float()
    w = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n,), generator=g)]
    return g, src, w


def _ref(dst, src, rows, F, w=None, src_row=None):
    ok = (dst >= 0) & (dst < rows)
    v = (src[src_row] if src_row is not None else src)[:, :F].double()
    if w is not None:
        v = v * w[:, None].double()
    ref = torch.zeros(rows, F, dtype=torch.float64)
    ref.index_add_(0, dst[ok], v[ok])
    return ref


def _assert_exact(out, ref, dst, rows, what):
    ok = (dst >= 0) & (dst < rows)
    assert ok.sum() == 0 or int(torch.bincount(dst[ok]).max()) <= 256, what      # the premise of exactness
    assert torch.equal(ref.float().double(), ref), what                         # the reference itself is exact in fp32
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(ref.shape), (what, out.dtype, out.shape)
    assert torch.equal(out.cpu(), ref.float()), (what, (out.cpu().double() - ref).abs().max().item())


def _hip(dst, src, rows, **kw):
    from pings_amd import neural_points as hnp

    kw = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    return hnp.rows_scatter_add(dst.cuda(), src if src.is_cuda else src.cuda(), rows, **kw)


def test_exact_inputs_stay_exact_and_both_sides_of_the_switch_are_reached():
    """CPU only: the integer / power-of-two inputs give an fp64 reference that fp32 holds exactly, and the row counts the
    cases use lie on the two sides of `4 * n_pairs < rows`."""
    n = 300
    for path in PATHS:
        rows = _rows_for(path, n)
        assert _takes_bucket_kernel(n, rows) == (path == "bucket")
        g, src, w = _exact_inputs(1, n, n, 67)
        dst = torch.randint(0, rows, (n,), generator=g)
        dst[:256] = 5                                               # the fullest row the cases use
        ref = _ref(dst, src, rows, 64, w)
        assert torch.equal(ref.float().double(), ref) and float(ref.abs().max()) > 256.0
    assert not _takes_bucket_kernel(1, 4) and _takes_bucket_kernel(1, 5) and _takes_bucket_kernel(0, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("F", F_ALL)
def test_every_lane_class_is_exact_on_both_kernels(F, path):
    """300 weighted pairs (two blocks of the pair-driven kernel, several of the row-driven one), a hot row with 200
    pairs, pairs on the last row, skipped pairs (-1 and >= rows); `ld == F` for even F and `ld == F + 3` for odd F."""
    n = 300
    rows = _rows_for(path, n)
    ld = F if F % 2 == 0 else F + 3
    g, src, w = _exact_inputs(100 + F, n, n, ld)
    dst = torch.randint(0, rows, (n,), generator=g)
    dst[10:210] = 7
    dst[210:220] = rows - 1
    dst[220:225] = -1
    dst[225:230] = rows
    dst[230] = rows + 12345
    out = _hip(dst, src, rows, w=w, F=F)
    _assert_exact(out, _ref(dst, src, rows, F, w), dst, rows, (F, path))


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_pair_counts_around_one_block(n, path):
    """Pair counts 0, 1 and around the 256-thread block of the histogram / placement / rank kernels; without weights.
    No pair at all always takes the zero-fill path (4 * 0 < rows)."""
    rows = max(1, _rows_for(path, n))
    F, ld = 5, 6
    g, src, _ = _exact_inputs(200 + n, n, max(n, 1), ld)
    src = src[:n]
    dst = torch.randint(0, rows, (n,), generator=g)
    if n:
        dst[-1] = rows - 1
    out = _hip(dst, src, rows, F=F)
    _assert_exact(out, _ref(dst, src, rows, F), dst, rows, (n, path))


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_every_pair_skipped_gives_zeros(path):
    n = 64
    rows = _rows_for(path, n)
    g, src, w = _exact_inputs(3, n, n, 8)
    dst = torch.tensor([-1, rows, -7, rows + 5] * (n // 4))
    assert bool(((dst < 0) | (dst >= rows)).all())
    out = _hip(dst, src, rows, w=w)
    assert out.shape == (rows, 8) and torch.equal(out.cpu(), torch.zeros(rows, 8))


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("row", ["first", "last"])
def test_all_pairs_on_one_row(row, path):
    """256 pairs in one bucket (the rank kernel's longest walk here), on row 0 or on row rows - 1."""
    n = 256
    rows = _rows_for(path, n)
    g, src, w = _exact_inputs(4, n, n, 13)
    dst = torch.full((n,), 0 if row == "first" else rows - 1)
    out = _hip(dst, src, rows, w=w)
    ref = _ref(dst, src, rows, 13, w)
    _assert_exact(out, ref, dst, rows, (row, path))
    assert int((out.cpu() != 0).any(1).sum()) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("F,extra", [(8, 0), (8, 5), (13, 0), (13, 1)])
def test_leading_dimension_equal_to_and_above_F(F, extra, path):
    n = 120
    rows = _rows_for(path, n)
    g, src, w = _exact_inputs(5, n, n, F + extra)
    src[:, F:] = 1000.0                                     # columns behind F must never be read into the sums
    dst = torch.randint(0, rows, (n,), generator=g)
    out = _hip(dst, src, rows, w=w, F=F)
    _assert_exact(out, _ref(dst, src, rows, F, w), dst, rows, (F, extra, path))


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("F", [4, 8, 61])
def test_source_is_a_column_slice_off_the_16_byte_grid(F, path):
    """`src` is `table[:, 1:]` of a row-major table: read where it lies, its first element 4 bytes behind an aligned
    address and the row pitch not a multiple of 16 bytes."""
    n = 150
    rows = _rows_for(path, n)
    g, full, w = _exact_inputs(6 + F, n, n, F + 3)
    dst = torch.randint(0, rows, (n,), generator=g)
    full_d = full.cuda()
    view = full_d[:, 1:]
    assert view.data_ptr() % 16 == 4 and view.stride(0) == F + 3 and not view.is_contiguous()
    out = _hip(dst, view, rows, w=w, F=F)
    _assert_exact(out, _ref(dst, full[:, 1:], rows, F, w), dst, rows, (F, path))


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_source_row_indirection(path):
    """Pair p reads row src_row[p] of a source with fewer rows than pairs (repeats, the last row, row 0)."""
    n, m, F = 257, 40, 20
    rows = _rows_for(path, n)
    g, src, w = _exact_inputs(7, n, m, F + 1)
    dst = torch.randint(0, rows, (n,), generator=g)
    sr = torch.randint(0, m, (n,), generator=g)
    sr[0], sr[1], sr[-1] = m - 1, 0, m - 1
    out = _hip(dst, src, rows, w=w, src_row=sr, F=F)
    _assert_exact(out, _ref(dst, src, rows, F, w, sr), dst, rows, path)
    out = _hip(dst, src, rows, src_row=sr, F=F)
    _assert_exact(out, _ref(dst, src, rows, F, None, sr), dst, rows, path)


@pytest.mark.gpu
@pytest.mark.parametrize("values", ["exact", "random"])
@pytest.mark.parametrize("F", [3, 8, 33])
def test_rows_padded_across_the_switch_give_the_same_bits(F, values):
    """The same pairs with the table padded from below the switch (row-driven kernel) to above it (pair-driven kernel):
    the rows both tables have are bitwise equal — the comment above `gather_bucket_kernel` promises the same order of
    additions — and every row no pair targets is exactly 0 in both."""
    n, used = 200, 300
    g, src, w = _exact_inputs(8 + F, n, n, F + 2)
    if values == "random":
        src, w = torch.randn(n, F + 2, generator=g), torch.rand(n, generator=g)
    dst = torch.randint(0, used, (n,), generator=g)
    dst[:60] = 11
    small, large = 4 * n, 4 * n + 1 + 513
    assert used <= small and not _takes_bucket_kernel(n, small) and _takes_bucket_kernel(n, large)
    a = _hip(dst, src, small, w=w, F=F).cpu()
    b = _hip(dst, src, large, w=w, F=F).cpu()
    assert torch.equal(a.view(torch.int32), b[:small].view(torch.int32))
    touched = torch.zeros(large, dtype=torch.bool)
    touched[dst] = True
    assert torch.equal(b[~touched].view(torch.int32), torch.zeros_like(b[~touched]).view(torch.int32))
    assert torch.equal(a[~touched[:small]].view(torch.int32), torch.zeros_like(a[~touched[:small]]).view(torch.int32))
    ref = _ref(dst, src, large, F, w)
    if values == "exact":
        _assert_exact(b, ref, dst, large, F)
    else:
        assert rel_err(b, ref) <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_random_values_within_the_project_bound_and_reproducible(path):
    """Random fp32 values and weights, a hot row of 3,000 pairs: within 1e-5 of fp64 (relative to the largest entry) and
    two identical calls give the same bits."""
    n = 6000
    rows = _rows_for(path, n)
    g = torch.Generator().manual_seed(9)
    dst = torch.randint(0, rows, (n,), generator=g)
    dst[:3000] = 17
    dst[torch.randint(0, n, (200,), generator=g)] = -1
    src, w = torch.randn(n, 19, generator=g), torch.rand(n, generator=g)
    a = _hip(dst, src, rows, w=w, F=16)
    b = _hip(dst, src, rows, w=w, F=16)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert rel_err(a, _ref(dst, src, rows, 16, w)) <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_plan_built_once_applied_to_two_tables(path):
    """`pings_rows_plan_build` once, `pings_rows_plan_apply` on two tables of different width (8 with ld 8, 13 with ld
    16, with and without weights): each result has the bits of `rows_scatter_add` on the same pairs, and equals fp64."""
    from pings_amd import _lib, neural_points as hnp

    L = _lib.lib()
    n = 257
    rows = _rows_for(path, n)
    g, src_a, w = _exact_inputs(10, n, n, 8)
    src_b = torch.randint(-64, 65, (n, 16), generator=g).float()
    dst = torch.randint(0, rows, (n,), generator=g)
    dst[:100] = rows - 1
    dst[100:104] = -1
    dst_d, w_d = dst.cuda(), w.cuda()
    plan = torch.empty(L.pings_rows_plan_bytes(n, rows), dtype=torch.uint8, device="cuda")
    _lib.check(L.pings_rows_plan_build(_lib.ptr(dst_d), n, rows, _lib.ptr(plan), _lib.stream_ptr(dst_d.device)),
               "pings_rows_plan_build")
    for src, F, wv in ((src_a, 8, w_d), (src_b, 13, None), (src_b, 13, w_d)):
        src_d = src.cuda()
        out = torch.full((rows, F), 7.0, device="cuda")             # stale content must be overwritten
        _lib.check(L.pings_rows_plan_apply(_lib.ptr(plan), n, rows, _lib.ptr(src_d), int(src.shape[1]), F,
                                           _lib.ptr(wv), _lib.ptr(out), _lib.stream_ptr(dst_d.device)),
                   "pings_rows_plan_apply")
        one = hnp.rows_scatter_add(dst_d, src_d, rows, w=wv, F=F)
        assert torch.equal(out.view(torch.int32), one.view(torch.int32)), (F, path)
        _assert_exact(out, _ref(dst, src, rows, F, w if wv is not None else None), dst, rows, (F, path))


@pytest.mark.gpu
@pytest.mark.parametrize("F", [0, 65])
def test_feature_widths_outside_1_to_64_are_refused(F):
    from pings_amd import _lib

    src = torch.zeros(8, 70, device="cuda")
    dst = torch.zeros(8, dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.PingsHipError):
        _hip(dst, src, 16, F=F)
    L = _lib.lib()
    plan = torch.empty(L.pings_rows_plan_bytes(8, 16), dtype=torch.uint8, device="cuda")
    _lib.check(L.pings_rows_plan_build(_lib.ptr(dst), 8, 16, _lib.ptr(plan), _lib.stream_ptr(dst.device)), "plan_build")
    out = torch.zeros(16, 70, device="cuda")
    with pytest.raises(_lib.PingsHipError):
        _lib.check(L.pings_rows_plan_apply(_lib.ptr(plan), 8, 16, _lib.ptr(src), 70, F, None, _lib.ptr(out),
                                           _lib.stream_ptr(dst.device)), "pings_rows_plan_apply")
