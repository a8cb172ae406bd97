"""The constructions of sparse_worst_cases.py, proved with Python integers on the host: what test_gpu_spmv_bounds.py and
test_gpu_algebra_bounds.py take for granted.  No GPU, no library: a construction that comes out short fails here, and a GPU test
never skips a case for it."""
import numpy as np
import pytest

import sparse_worst_cases as W

SMALL = [65521, 32749]
LARGE = [65537, 0xFFFFFFFB]


def ints(a):
    return [int(v) for v in a]


def dense_rows(M, p):
    """row -> {column: sum mod p} in Python integers"""
    out = []
    for i in range(M.n):
        d = {}
        for k in range(int(M.ptr[i]), int(M.ptr[i + 1])):
            d[int(M.j[k])] = (d.get(int(M.j[k]), 0) + int(M.v[k])) % p
        out.append(d)
    return out


def rows_of_canon(want, p):
    ptr, j, x = want[:3]
    assert np.all(x != 0) and np.all(2 * np.abs(x.astype(np.int64)) <= p)
    rows = []
    for i in range(len(ptr) - 1):
        cols = ints(j[ptr[i]:ptr[i + 1]])
        assert cols == sorted(set(cols))
        rows.append({c: int(v) % p for c, v in zip(cols, x[ptr[i]:ptr[i + 1]])})
    return rows


def test_restated_rules():
    assert [W.spg_class_of(b) for b in (-1, 0, 1, 32, 33, 64, 65, 128, 129, 4096, 4097, 2**40)] == [9, 9, 0, 0, 1, 1, 2, 2, 3, 7, 8, 8]
    assert [W.spg_lanes(c) for c in range(10)] == [16, 64, 64, 64, 64, 256, 256, 256, 256, 0]
    assert W.hash_home(1, 7) == 2654435761 >> 25 and W.hash_home(3, 13) == ((3 * 2654435761) % 2**32) >> 19
    assert np.array_equal(W.hash_home(np.arange(1000), 9), [W.hash_home(c, 9) for c in range(1000)])
    assert [W.spmv_team(kw) for kw in (1, 2, 4, 8, 16, 32, 64)] == [8, 16, 32, 64, 64, 64, 64]
    assert W.spmv_chunks(1) == [(1, 1)] and W.spmv_chunks(5) == [(8, 5)] and W.spmv_chunks(64) == [(64, 64)]
    assert W.spmv_chunks(65) == [(64, 64), (1, 1)] and W.spmv_chunks(129) == [(64, 64), (64, 64), (1, 1)]
    # the block widths reach every kernel width full (kc == kw), partly filled, and a second chunk of one column
    seen = {c for k in W.SPMV_BLOCKS for c in W.spmv_chunks(k)}
    assert {(kw, kw) for kw in (1, 2, 4, 8, 16, 32, 64)} <= seen
    assert {(4, 3), (8, 5), (32, 17), (64, 33), (64, 63)} <= seen
    assert W.spmv_chunks(65)[1] == (1, 1) and W.spmv_chunks(129)[2] == (1, 1)


def test_edge_lists_hold_both_sides():
    L = W.SPMV_LENGTHS
    for edge in (W.SPMV_SHORT, W.SPMV_SEG):
        assert edge in L and edge + 1 in L and edge - 1 in L
    assert 0 in L and 1 in L and 2 * W.SPMV_SEG in L and 2 * W.SPMV_SEG + 1 in L
    bins = [W.spmv_bin(l) for l in L]
    assert bins.count("short") == 4 and bins.count("medium") == 6 and bins.count("long") == 3
    for name in ("short", "medium", "long"):  # no list is a range of rows: each bin's rows are interleaved with the others'
        idx = [i for i, b in enumerate(bins) if b == name]
        assert idx != list(range(idx[0], idx[0] + len(idx)))
    assert W.SPG_EDGES == [32, 64, 128, 256, 512, 1024, 2048, 4096]
    bounds = {b for E in W.SPG_EDGES for b in (E, E + 1)}
    assert {32, 33} <= bounds
    for c in range(7):
        assert (64 << c) in bounds and (64 << c) + 1 in bounds
        assert W.spg_class_of(64 << c) == 1 + c and W.spg_class_of((64 << c) + 1) == 2 + c
    assert W.spg_class_of(32) == 0 and W.spg_class_of(33) == 1
    assert sorted(W.BINNED_STORED) == [33, 16385, 32769]


@pytest.mark.parametrize("p", SMALL + LARGE)
@pytest.mark.parametrize("sign", [1, -1])
def test_designed_pairs(p, sign):
    rng = np.random.default_rng(p % 1000 + sign)
    t = W.target_residue(p, sign)
    assert abs(t) == (p // 2 - 512 if p < 2**16 else p // 2 - 1) and (t > 0) == (sign > 0)
    a, x = W.designed_pairs(p, 3000, rng, sign)
    assert np.all(a != 0) and np.all(2 * np.abs(a) <= p) and np.all(2 * np.abs(x) <= p)
    assert all((u * v - t) % p == 0 for u, v in zip(ints(a), ints(x)))
    assert sum(u * v for u, v in zip(ints(a), ints(x))) % p == (3000 * t) % p
    # the unreduced twins: inside int32, congruent, and really unreduced where int32 has room for one more p
    rng2 = np.random.default_rng(p % 1000 + sign)
    a2, x2 = W.designed_pairs(p, 3000, rng2, sign, unreduced=0.1)
    assert np.array_equal(a2, a)
    assert x2.min() >= W.INT32_MIN and x2.max() <= W.INT32_MAX
    assert all((u - v) % p == 0 for u, v in zip(ints(x2), ints(x)))
    moved = int((x2 != x).sum())
    assert moved <= 500
    if p < 2**31:
        assert moved >= 200 and np.all(2 * np.abs(x2[x2 != x]) > p)


@pytest.mark.parametrize("p", SMALL + LARGE)
def test_lane_worst_case(p):
    for sign in (1, -1):
        rng = np.random.default_rng(p % 1000 + 5 + sign)
        t = W.target_residue(p, sign)
        M, x, sums = W.lane_worst_case(p, rng, sign)
        assert M.n == 3 and M.m == 81921 and ints(W.row_lengths(M)) == W.LANE_ROWS == [16384, 49153, 81921]
        assert [W.spmv_bin(l) for l in W.LANE_ROWS] == ["medium", "long", "long"] and all(l % W.SPMV_SEG == 1 for l in W.LANE_ROWS[1:])
        assert np.all(M.v != 0) and np.all(x != 0) and np.all(2 * np.abs(M.v) <= p)
        prod = ((M.v % p).astype(np.uint64) * (x[M.j] % p).astype(np.uint64)) % np.uint64(p)  # < p^2 < 2^64
        prod = prod.astype(np.int64)
        tt = t % p
        # the medium row: every product is t; a lane that takes the row whole sums 16384 t
        assert np.all(prod[:16384] == tt) and len(set(ints(M.j[:16384]))) == 16384
        assert sums[0] == 16384 * t and int(prod[:16384].sum()) % p == sums[0] % p
        # the long rows: segment s holds the columns [s SEG, (s + 1) SEG), every product but its last is t, its sum is t
        for i in (1, 2):
            lo, hi = int(M.ptr[i]), int(M.ptr[i + 1])
            nseg = -(-(hi - lo) // W.SPMV_SEG)
            assert nseg == (4, 6)[i - 1]
            for s in range(nseg):
                seg = slice(lo + s * W.SPMV_SEG, min(lo + (s + 1) * W.SPMV_SEG, hi))
                cols = M.j[seg]
                assert np.array_equal(np.sort(cols), np.arange(s * W.SPMV_SEG, s * W.SPMV_SEG + len(cols)))
                assert len(cols) == 1 or not np.array_equal(np.sort(cols), cols)
                assert np.all(prod[seg][:-1] == tt) and sum(ints(prod[seg])) % p == tt
            assert sums[i] % p == sum(ints(prod[lo:hi])) % p == (nseg * t) % p
        # magnitudes: what a lane's accumulator reaches, against its type
        if p < 2**16:
            assert 16384 * (abs(t) + 256) < 2**31
            if p == 65521:
                assert 2**28.97 < 16384 * abs(t) < 2**28.98
                assert 49153 * abs(t) < 2**31 < (81921 - 5) * abs(t) - 5 * (p // 2)  # only the longest row needs the cut into segments
        else:
            assert 16384 * abs(t) < 2**63 and abs(t) == p // 2 - 1


@pytest.mark.parametrize("p", [3, 65521, 65537, 0xFFFFFFFB])
def test_spmv_matrices(p):
    rng = np.random.default_rng(p % 1000 + 11)
    A = W.spmv_designed(p, rng)
    assert (A.n, A.m) == (13, 32769) and ints(W.row_lengths(A)) == W.SPMV_LENGTHS and len(A.j) == 114978
    for i in range(A.n):
        cols = ints(A.j[A.ptr[i]:A.ptr[i + 1]])
        assert len(set(cols)) == len(cols) and (len(cols) < 8 or cols != sorted(cols))
    assert np.all(A.v != 0) and np.all(2 * np.abs(A.v) <= p)
    T = W.host_transpose(A)
    assert (T.n, T.m) == (A.m, A.n) and W.row_lengths(T).max() <= 13 and W.row_lengths(T).min() >= 1
    back = W.host_transpose(T)
    assert dense_rows(back, 2**40) == dense_rows(A, 2**40)
    S1 = W.spmv_short_plus_one(p, rng)
    l1 = ints(W.row_lengths(S1))
    assert sorted(l1) == sorted(list(range(33)) + [40]) and [W.spmv_bin(l) for l in l1].count("medium") == 1 and l1[0] == 0 and l1[-1] == 32
    # rows binned longer than they are
    Bn = W.binned_longer(p, rng)
    assert ints(W.row_lengths(Bn)) == W.BINNED_STORED and [W.spmv_bin(l) for l in W.BINNED_STORED] == ["medium", "long", "long"]
    assert Bn.v.min() >= W.INT32_MIN and Bn.v.max() <= W.INT32_MAX
    for i in range(Bn.n):
        v = Bn.v[Bn.ptr[i]:Bn.ptr[i + 1]]
        live = np.flatnonzero(v % p)
        assert len(live) == 5 and live[0] == 0 and live[-1] == len(v) - 1
    if p < 2**31:
        assert np.count_nonzero(Bn.v[Bn.v % p == 0]) > 1000 and np.all(2 * np.abs(Bn.v[Bn.v % p != 0]) > p)


def test_ref_apply_against_python_integers():
    rng = np.random.default_rng(3)
    for p in (3, 65521, 0xFFFFFFFB):
        A = W.rows_of_lengths([0, 5, 40, 1, 33], 50, rng, lambda l: W.lift(W.rand_values(p, l, rng), p, rng, 0.3))
        for trans in (False, True):
            rin, rout = (A.n, A.m) if trans else (A.m, A.n)
            X, Y = W.rand_int32(rng, (rin, 3)), W.rand_int32(rng, (rout, 3))
            want = [[int(Y[i, c]) for c in range(3)] for i in range(rout)]
            for i in range(A.n):
                for k in range(int(A.ptr[i]), int(A.ptr[i + 1])):
                    src, dst = (i, int(A.j[k])) if trans else (int(A.j[k]), i)
                    for c in range(3):
                        want[dst][c] += int(A.v[k]) * int(X[src, c])
            got = W.ref_apply(A.ptr, A.j, A.v, X, Y, trans, p)
            assert got.dtype == np.int32 and np.all(2 * np.abs(got.astype(np.int64)) <= p)
            assert all((int(got[i, c]) - want[i][c]) % p == 0 for i in range(rout) for c in range(3))
            # the transpose applied the other way round is the same product
            T = W.host_transpose(A)
            assert np.array_equal(W.ref_apply(T.ptr, T.j, T.v, X, Y, not trans, p), got)


def test_algebra_references_against_python_integers():
    rng = np.random.default_rng(4)
    for p in (3, 65521, 0xFFFFFFFB):
        vals = lambda l: W.lift(W.rand_values(p, l, rng), p, rng, 0.3)
        A = W.rows_of_lengths([3, 0, 7, 10, 1], 12, rng, vals)
        B = W.rows_of_lengths([0, 4, 9, 2, 1, 0, 5, 9, 9, 3, 1, 2], 9, rng, vals)
        da, db = dense_rows(A, p), dense_rows(B, p)
        want = []
        for i in range(A.n):
            d = {}
            for k, a in da[i].items():
                for c, b in db[k].items():
                    d[c] = (d.get(c, 0) + a * b) % p
            want.append({c: v for c, v in d.items() if v})
        assert rows_of_canon(W.ref_mul(A, B, p), p) == want
        A2 = W.rows_of_lengths([3, 0, 7, 10, 1], 12, rng, vals)
        sa, sb = W.LINCOMB_SCALARS
        d2 = dense_rows(A2, p)
        want = [{c: (sa * da[i].get(c, 0) + sb * d2[i].get(c, 0)) % p for c in set(da[i]) | set(d2[i])} for i in range(A.n)]
        assert rows_of_canon(W.ref_lincomb(sa, A, sb, A2, p), p) == [{c: v for c, v in d.items() if v} for d in want]
        assert rows_of_canon(W.ref_lincomb(1, A, 0, None, p), p) == [{c: v for c, v in d.items() if v} for d in da]
        want = [{c - 2: v for c, v in da[i].items() if 2 <= c < 9 and v} for i in range(1, 4)]
        assert rows_of_canon(W.ref_submatrix(A, 1, 4, 2, 9, p), p) == want


@pytest.mark.parametrize("E", W.SPG_EDGES)
def test_class_edge_cases(E):
    for p in (65521, 0xFFFFFFFB):
        t = W.target_residue(p)
        for pad in (True, False):
            rng = np.random.default_rng(E + p % 1000)
            A, B, bounds = W.class_edge_product(E, p, rng, pad)
            nnz = len(A.j)
            assert (nnz <= 8 * A.n) == pad and B.m == W.SPG_M and A.m == B.n
            assert ints(W.product_bounds(A, B)) == bounds and bounds[:7] == [E, E + 1, E, E + 1, E, E + 1, E] and max(bounds) == E + 1
            assert [W.spg_class_of(b) for b in bounds[:2]] == [W.spg_class_of(E), W.spg_class_of(E) + 1]
            want = W.ref_mul(A, B, p)
            rows = rows_of_canon(want, p)
            assert want[3] == 2 * E + 1 + (A.n - 2)  # distinct keys: rows 0 and 1 in full, one column in every other row
            assert len(rows[0]) == E and len(rows[1]) == E + 1  # all columns distinct
            for i in (0, 1):
                cols = ints(np.concatenate([B.j[B.ptr[k]:B.ptr[k + 1]] for k in A.j[A.ptr[i]:A.ptr[i + 1]]]))
                assert len(set(cols)) == len(cols) and cols != sorted(cols)
            star = int(B.j[B.ptr[3]])
            assert rows[2] == {star: (E * t) % p} and rows[3] == {star: ((E + 1) * t) % p} and rows[6] == {star: (-E * t) % p}
            assert rows[4] == {} and rows[5] == {}
            # every term of rows 2, 3, 6 is the designed product
            x = {3 + k: int(B.v[B.ptr[3 + k]]) for k in range(E + 1)}
            for i, s in ((2, 1), (3, 1), (6, -1)):
                assert all((int(v) * x[int(k)] - s * t) % p == 0 for k, v in zip(A.j[A.ptr[i]:A.ptr[i + 1]], A.v[A.ptr[i]:A.ptr[i + 1]]))
            if p < 2**16:
                assert (E + 1) * (abs(t) + 256) < 2**31  # the i32 slot
        rng = np.random.default_rng(E + p % 1000 + 1)
        LA, LB, sa, sb, bounds = W.class_edge_lincomb(E, p, rng)
        assert sa % p and sb % p and LA.n == LB.n == 6 and bounds == [E] * 3 + [E + 1] * 3
        assert ints(W.row_lengths(LA) + W.row_lengths(LB)) == bounds
        rows = rows_of_canon(W.ref_lincomb(sa, LA, sb, LB, p), p)
        assert [len(r) for r in rows] == [E, E - 2 * (E // 4), E, E + 1, E + 1 - 2 * (E // 4), E + 1]
        for i in (1, 4):
            shared = set(ints(LA.j[LA.ptr[i]:LA.ptr[i + 1]])) & set(ints(LB.j[LB.ptr[i]:LB.ptr[i + 1]]))
            assert len(shared) == E // 4 and not shared & set(rows[i])
        Sm, windows, bounds = W.class_edge_submatrix(E, p, rng)
        assert ints(W.row_lengths(Sm)) == bounds == [E, E + 1, 0, E + 1, E]
        kept = [int(W.ref_submatrix(Sm, 0, Sm.n, c0, c1, p)[0][-1]) for c0, c1 in windows]
        assert kept[0] == 4 * E + 2 and kept[2] == 0 and 0 < kept[1] < kept[0]


@pytest.mark.parametrize("p", [3, 65521, 0xFFFFFFFB])
def test_segment_batch_case(p):
    rng = np.random.default_rng(p % 1000 + 21)
    A, B, lanes, bounds = W.segment_batch_case(p, rng)
    lb = W.row_lengths(B)
    assert set(ints(lb[:-1])) == {0, 1, 2, 3} and lb[-1] == W.SEG_B_LONG
    assert ints(W.product_bounds(A, B)) == bounds
    assert [W.spg_lanes(W.spg_class_of(b)) for b in bounds] == lanes  # every row is taken with the batch size it was laid out for
    la = ints(W.row_lengths(A))
    assert set(la) >= {63, 64, 65, 255, 256, 257, 513, 1025}
    assert {(n, bs) for n, bs in zip(la, lanes)} >= {(n, 64) for n in (63, 64, 65, 255, 256, 257, 513)} | {(n, 256) for n in (255, 256, 257, 513, 1025)}
    assert W.spg_class_of(max(bounds)) == W.SPG_CLS_GLOBAL and 0 in bounds
    first = last = run = whole = lone = 0
    for i in range(A.n):
        bs = lanes[i]
        if bs < 64:
            continue
        seg = lb[A.j[A.ptr[i]:A.ptr[i + 1]]]
        n = len(seg)
        for s0 in range(0, n, bs):
            batch = seg[s0:s0 + bs]
            if batch.sum() == 0:
                whole += len(batch) == bs
                lone += len(batch) < bs
                continue
            first += batch[0] == 0
            last += batch[-1] == 0
            if s0 + bs < n:
                run += batch[-1] == 0 and batch[-2] == 0 and seg[s0 + bs] == 0
    assert first >= 4 and last >= 4 and run >= 3 and whole >= 6 and lone >= 2
    tail = lb[A.j[A.ptr[A.n - 1]:A.ptr[A.n]]]
    assert tail[:-1].sum() == 0 and tail[-1] == 40 and bounds[-2] == 3 and bounds[-3] == 0
    if p == 3:
        want = W.ref_mul(A, B, p)
        assert int(want[0][-1]) < want[3], "no sum cancels"


@pytest.mark.parametrize("logt", [7, 13])
def test_probe_chain_case(logt):
    half = 1 << (logt - 1)
    m = W.PROBE_M[logt]
    cols = W.colliding_columns(logt, half, m)
    assert len(cols) == half and len(set(ints(cols))) == half and cols.max() < m and cols.min() >= 0
    assert all(W.hash_home(int(c), logt) == (1 << logt) - 1 for c in cols)
    assert np.array_equal(cols, [c for c in range(int(cols[min(half, 40) - 1]) + 1) if W.hash_home(c, logt) == (1 << logt) - 1][:40] + ints(cols[40:]))
    assert len(W.colliding_columns(logt, half, 1000)) < half  # a short construction shows
    for p in (65521, 0xFFFFFFFB):
        A, B, bounds = W.probe_chain_case(logt, p, np.random.default_rng(logt))
        assert B.m == m and ints(W.product_bounds(A, B)) == bounds == [half] * 3
        assert W.spg_class_of(half) == logt - 6 and W.spg_paths(bounds) == (0, 3, 0)
        assert set(ints(B.j)) <= set(ints(cols)) and len(B.j) == 3 * half
        r0 = ints(B.j[B.ptr[0]:B.ptr[1]])
        assert r0 == sorted(r0, reverse=True) and len(set(r0)) == half
        assert ints(B.j[B.ptr[1]:B.ptr[2]]) == ints(B.j[B.ptr[2]:B.ptr[3]])[::-1]
        quarters = [ints(B.j[B.ptr[k]:B.ptr[k + 1]]) for k in range(3, 7)]
        assert all(sorted(q) == sorted(quarters[0]) for q in quarters) and len({tuple(q) for q in quarters}) == 4


@pytest.mark.parametrize("p", [65521, 0xFFFFFFFB])
def test_tiny_capacity_cases(p):
    rng = np.random.default_rng(p % 1000 + 31)
    t = W.target_residue(p)
    A, B, bounds = W.tiny_capacity_case(p, rng)
    assert A.n == W.TINY_ROWS > 2 * 16 and W.TINY_ROWS % 16 and ints(W.product_bounds(A, B)) == bounds == [32] * A.n
    assert W.spg_paths(bounds) == (A.n, 0, 0)
    rows = rows_of_canon(W.ref_mul(A, B, p), p)
    assert rows[0] == {77: (32 * t) % p} and rows[1] == {} and len(rows[2]) == 32 and len(rows[3]) == 24
    d = ints(B.j[B.ptr[32]:B.ptr[33]])
    assert d == sorted(d, reverse=True) and len(set(d)) == 32
    assert len(set(ints(B.j[B.ptr[33]:B.ptr[34]])) & set(ints(B.j[B.ptr[34]:B.ptr[35]]))) == 8
    Sm, (c0, c1), bounds = W.tiny_capacity_submatrix(p, rng)
    assert ints(W.row_lengths(Sm)) == bounds == [32] * W.TINY_ROWS
    for i in range(Sm.n):
        inside = [c0 <= c < c1 for c in ints(Sm.j[Sm.ptr[i]:Sm.ptr[i + 1]])]
        if i % 5 == 4:
            assert not any(inside)
        else:
            assert inside == [(k + i) % 2 == 0 for k in range(32)]
    assert [len(r) for r in rows_of_canon(W.ref_submatrix(Sm, 0, Sm.n, c0, c1, p), p)] == [0 if i % 5 == 4 else 16 for i in range(Sm.n)]
