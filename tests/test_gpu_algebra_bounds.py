"""The row classes of the exact matrix algebra (csrc/spgemm.hpp, spg_run in engine.hip) on inputs built so that one named piece
must be right: rows on both sides of every class edge (table at its full permitted load, the sort without padding, the most
lazy terms on one slot), the segment-batch loop with empty segments wherever a batch can hold them, probe chains that start at the
last slot and wrap, tiny rows at exactly 32 terms.

The inputs and the exact integer references come from sparse_worst_cases.py; test_sparse_worst_cases_host.py proves the
constructions (bounds, classes, designed products, home slots) without a GPU.  Every result is compared entry for entry in
canonical form (same(): nnz == nzmax, row pointers, columns, values)."""
import numpy as np
import pytest

import sparse_worst_cases as W
from test_gpu_algebra import same

pytestmark = pytest.mark.gpu

PRIMES = [65521, 0xFFFFFFFB]


def to_csr(S, M, p):
    return S.CSR.from_arrays(M.n, M.m, M.ptr, M.j.astype(np.int32), M.v.astype(np.int32), prime=p)


def paths(st):
    return st["rows_tiny"], st["rows_hash"], st["rows_global"]


@pytest.mark.parametrize("p", PRIMES)
@pytest.mark.parametrize("E", W.SPG_EDGES)
def test_rows_on_every_class_edge(S, E, p):
    """Rows of bound exactly E and E + 1 for E = 32, 64, .., 4096 (class_edge_product / _lincomb / _submatrix): all columns
    distinct and unsorted (bound 64 << c: the table half full, L == LIST, the bitonic sort without padding; one more: the next
    class), and all terms on one column with designed products (E = 4096, p = 65521: 4096 lazy terms of 32248 on one i32 slot,
    2^26.98), one twin summing to 0.  stats() must agree with the restated spg_class_of.  The product runs twice, sized by
    k_spg_size (A padded to nnz <= 8 n) and by k_spg_size_wave."""
    seed = E + p % 1000
    made = {}
    for pad in (True, False):
        A, B, bounds = W.class_edge_product(E, p, np.random.default_rng(seed), pad)
        want = W.ref_mul(A, B, p)
        with S.DeviceCSR(to_csr(S, A, p)) as a, S.DeviceCSR(to_csr(S, B, p)) as b:
            c = a @ b
        st = c.stats()
        assert paths(st) == W.spg_paths(bounds), (E, p, pad, st)
        assert st["max_bound"] == E + 1 and st["flops"] == sum(bounds) and st["entries"] == int(want[0][-1]) == c.nnz
        same(c.download(), want, (E, p, pad))
        made[pad] = c
        if not pad:
            same(to_csr(S, A, p) @ to_csr(S, B, p), want, (E, p, "one-shot"))
    first = made[True][0:7, :]
    assert first.equals(made[False]) and made[False].equals(first)
    for c in (first, made[True], made[False]):
        c.close()

    # a A + b B
    A, B, sa, sb, bounds = W.class_edge_lincomb(E, p, np.random.default_rng(seed + 1))
    with S.DeviceCSR(to_csr(S, A, p)) as a, S.DeviceCSR(to_csr(S, B, p)) as b:
        c = a.lincomb(sa, sb, b)
        want = W.ref_lincomb(sa, A, sb, B, p)
        assert paths(c.stats()) == W.spg_paths(bounds) and c.stats()["max_bound"] == E + 1
        assert int(want[0][-1]) == want[3] - 2 * (E // 4), "the overlap cancels"
        same(c.download(), want, (E, p, "lincomb"))
        same((a + b).download(), W.ref_lincomb(1, A, 1, B, p), (E, p, "sum"))
        c1 = b.lincomb(sb)  # one segment per row: bounds E + 1, E + 1, E + 1 and E, E
        assert paths(c1.stats()) == W.spg_paths(W.row_lengths(B))
        same(c1.download(), W.ref_lincomb(sb, B, 0, None, p), (E, p, "scaled"))

    # A[r0:r1, c0:c1]
    A, windows, bounds = W.class_edge_submatrix(E, p, np.random.default_rng(seed + 2))
    with S.DeviceCSR(to_csr(S, A, p)) as a:
        for c0, c1 in windows:
            d = a[0:A.n, c0:c1]
            want = W.ref_submatrix(A, 0, A.n, c0, c1, p)
            assert d.shape == (A.n, c1 - c0) and paths(d.stats()) == W.spg_paths(bounds) and d.stats()["max_bound"] == E + 1
            same(d.download(), want, (E, p, c0, c1))
        d = a[1:4, 1000:3048]
        same(d.download(), W.ref_submatrix(A, 1, 4, 1000, 3048, p), (E, p, "rows 1:4"))
        assert a[0:A.n, W.SUBMATRIX_FREE:W.SUBMATRIX_FREE + 100].nnz == 0  # the window that keeps nothing


@pytest.mark.parametrize("p", [3] + PRIMES)
def test_segment_batches(S, p):
    """Product rows of 63 .. 2049 segments of 0 .. 3 terms (segment_batch_case): the s0 += BS loop of spg_for_terms in the 64-lane
    and the 256-lane hash classes and in the global class, with empty rows of B first and last in a batch, in runs across a batch
    edge and as whole batches (total == 0); a row all of whose segments are empty, and rows with one non-empty segment, the last"""
    A, B, lanes, bounds = W.segment_batch_case(p, np.random.default_rng(p % 1000 + 21))
    want = W.ref_mul(A, B, p)
    with S.DeviceCSR(to_csr(S, A, p)) as a, S.DeviceCSR(to_csr(S, B, p)) as b:
        c = a @ b
        st = c.stats()
        assert paths(st) == W.spg_paths(bounds) and st["rows_global"] == 1 and st["flops"] == sum(bounds) and st["max_bound"] == max(bounds), st
        same(c.download(), want, p)
    if p == 3:
        assert int(want[0][-1]) < want[3]  # sums cancel


@pytest.mark.parametrize("p", PRIMES)
@pytest.mark.parametrize("logt", [7, 13])
def test_probe_chains_that_wrap(S, logt, p):
    """Rows of bound 2^(LOGT - 1) whose columns all have the last slot of the table as home (probe_chain_case): the chain wraps to
    slot 0 and is as long as the table's load allows (64 of 128 slots, 4096 of 8192); columns met again in another order are found
    at the end of a long probe.  m is about 2^14 and 2^26: no row may fall in the global class."""
    A, B, bounds = W.probe_chain_case(logt, p, np.random.default_rng(logt))
    want = W.ref_mul(A, B, p)
    with S.DeviceCSR(to_csr(S, A, p)) as a, S.DeviceCSR(to_csr(S, B, p)) as b:
        c = a @ b
        st = c.stats()
        assert st["rows_global"] == 0 and paths(st) == W.spg_paths(bounds) == (0, 3, 0) and st["max_bound"] == 1 << (logt - 1), st
        same(c.download(), want, (logt, p))


@pytest.mark.parametrize("p", PRIMES)
def test_tiny_rows_at_capacity(S, p):
    """37 rows of bound exactly 32 = SPG_TINY (tiny_capacity_case): 32 designed terms on one column and a twin that cancels, 32
    distinct columns stored descending, 16 + 16 with 8 shared columns; the submatrix form with in-window and out-of-window terms
    alternating and rows entirely outside the window.  37 rows: two workgroups with 16 busy teams, one with 5."""
    A, B, bounds = W.tiny_capacity_case(p, np.random.default_rng(p % 1000 + 31))
    with S.DeviceCSR(to_csr(S, A, p)) as a, S.DeviceCSR(to_csr(S, B, p)) as b:
        c = a @ b
        assert paths(c.stats()) == (W.TINY_ROWS, 0, 0) and c.stats()["max_bound"] == 32
        same(c.download(), W.ref_mul(A, B, p), p)
    M, (c0, c1), bounds = W.tiny_capacity_submatrix(p, np.random.default_rng(p % 1000 + 32))
    with S.DeviceCSR(to_csr(S, M, p)) as a:
        d = a[0:M.n, c0:c1]
        assert paths(d.stats()) == (W.TINY_ROWS, 0, 0)
        same(d.download(), W.ref_submatrix(M, 0, M.n, c0, c1, p), p)
        e = a[3:30, c0:c1]
        same(e.download(), W.ref_submatrix(M, 3, 30, c0, c1, p), p)
