"""GPU tests of block Wiedemann (spasm_amd_block_sequence / _dev, _block_berlekamp_massey, _block_wiedemann_det*;
csrc/block_krylov.hpp, csrc/block_bm.hpp).  The sequence is compared byte for byte with the restatement in Python integers
(tests/block_wiedemann_ref.py); for the matrix with a long row, whose dense form no Python loop can walk, with the exact numpy
products of tests/wiedemann_ref.py, which the small cases tie to the Python integers.  The generator is checked by its contract:
(A) annihilation, (B) row-reduced, (C) the row degrees of the reference, whose sum the reference alone ties to the rank of the block
Hankel matrix.  The determinant is compared with S.det (elimination) wherever status is 1."""
import ctypes as C
import functools

import numpy as np
import pytest

import block_wiedemann_ref as R
import wiedemann_ref as W
from wiedemann_ref import bal

pytestmark = pytest.mark.gpu

P3, P16, P32 = 3, 65521, 4294967291
PRIMES3 = (P3, P16, P32)
WIDTHS = (2, 4, 8, 16)
SLACK = 2   # len = 2 * ceil(n / b) + SLACK (include/spasm_amd.h)


def terms(n, b):
    return 2 * -(-n // b) + SLACK


def rand_bal(rng, shape, p):
    return bal(rng.integers(0, p, size=shape, dtype=np.int64), p)


def np_block_sequence(M, U, V, length, p, trans=False, d=None):
    """(length, b, b) balanced int32 by exact numpy int64 arithmetic: products below 2^32 each, sums of n of them below 2^63"""
    A = M.transpose() if trans else M
    Ur = np.asarray(U, dtype=np.int64) % p
    X = np.asarray(V, dtype=np.int64) % p
    dd = None if d is None else (np.asarray(d, dtype=np.int64) % p)[:, None]
    b = Ur.shape[1]
    out = np.zeros((length, b, b), dtype=np.int64)
    for i in range(length):
        if i:
            X = A.apply(X, p)
            if dd is not None:
                X = W.mulmod(np.broadcast_to(dd, X.shape).copy(), X, p)
        for r in range(b):
            out[i, r] = W.mulmod(np.broadcast_to(Ur[:, r:r + 1], X.shape).copy(), X, p).sum(axis=0) % p
    return bal(out, p)


def dense_of(M):
    D = [[0] * M.m for _ in range(M.n)]
    for i in range(M.n):
        for k in range(int(M.ptr[i]), int(M.ptr[i + 1])):
            D[i][int(M.j[k])] += int(M.v[k])
    return D


def short_rows_matrix(rng, n, p, empty=False):
    """rows of 0 .. 6 entries; with empty, rows 0, 5 and the last one are empty and so is a third of the others"""
    rows = []
    for i in range(n):
        l = min(n, int(rng.integers(1, 7)))
        if empty and (i in (0, 5, n - 1) or rng.random() < 0.33):
            l = 0
        cols = rng.choice(n, size=l, replace=False)
        rows.append([(int(c), int(v)) for c, v in zip(cols, rng.integers(1, p, size=l))])
    return W.Mat.from_rows(rows, n)


def long_row_matrix(rng, n, p):
    """row 3 has 16385 entries (two segments, the second of one entry: the segment and combine kernels), row 9 has 40 (a medium
    row), the others 0 .. 3"""
    rows = []
    for i in range(n):
        l = 16385 if i == 3 else 40 if i == 9 else int(rng.integers(0, 4))
        cols = rng.choice(n, size=l, replace=False)
        rows.append(list(zip(cols.tolist(), rng.integers(1, p, size=l).tolist())))
    return W.Mat.from_rows(rows, n)


# ---------------------------------------------------------------- the sequence
@pytest.mark.parametrize("d_given", (False, True))
@pytest.mark.parametrize("trans", (False, True))
@pytest.mark.parametrize("b", (2, 16))
@pytest.mark.parametrize("p", PRIMES3)
def test_sequence_matches_the_python_integers_on_short_rows(S, p, b, trans, d_given):
    rng = np.random.default_rng(31 * b + p % 1009 + 2 * int(trans) + int(d_given))
    n, length = 70, 5
    for empty in (False, True):
        M = short_rows_matrix(rng, n, p, empty=empty)
        # unreduced int32 words in U and V, the extremes among them
        U = rng.integers(-2**31, 2**31, size=(n, b), dtype=np.int64).astype(np.int32)
        V = rng.integers(-2**31, 2**31, size=(n, b), dtype=np.int64).astype(np.int32)
        U[0, 0], U[1, 0], V[0, 0], V[1, 0] = 2**31 - 1, -2**31, -2**31, 2**31 - 1
        d = rand_bal(rng, n, p) if d_given else None
        if d is not None:
            d[d == 0] = 1
        ref = R.block_sequence(dense_of(M), U.tolist(), V.tolist(), length, p, trans=trans, d_left=None if d is None else d.tolist())
        want = bal(np.array(ref, dtype=object), p)
        assert np_block_sequence(M, U, V, length, p, trans, d).tolist() == want.tolist()   # ties the numpy products to the integers
        U0, V0 = U.copy(), V.copy()
        with S.SpMV(M.csr(S, p)) as op:
            got = S.block_sequence(op, U, V, length, trans=trans, d_left=d)
            again = op.block_sequence(U, V, length, trans=trans, d_left=d)
            diag = S.krylov_sequence(op, U, V, length, trans=trans) if d is None else None
        assert got.shape == (length, b, b) and got.dtype == np.int32
        assert got.tobytes() == want.tobytes()
        assert again.tobytes() == got.tobytes()
        assert U.tobytes() == U0.tobytes() and V.tobytes() == V0.tobytes()
        st = S.block_stats()
        assert (st["b"], st["len"], st["steps"], st["n"]) == (b, length, length - 1, n)
        if diag is not None:   # the diagonal of a term is the scalar projection of the same U, V
            assert np.einsum("ijj->ij", got).tolist() == diag.tolist()


@pytest.mark.parametrize("b,p,trans,d_given", [(2, P3, False, True), (16, P16, False, False), (16, P32, False, True), (2, P32, True, False),
                                               (16, P3, True, True), (2, P16, True, False)])
def test_sequence_with_a_long_row_takes_the_segments_and_the_combine(S, p, b, trans, d_given):
    rng = np.random.default_rng(7 * b + p % 1013)
    n, length = 16500, 3
    M = long_row_matrix(rng, n, p)
    U, V = rand_bal(rng, (n, b), p), rand_bal(rng, (n, b), p)
    d = rand_bal(rng, n, p) if d_given else None
    if d is not None:
        d[d == 0] = 1
    want = np_block_sequence(M, U, V, length, p, trans, d)
    with S.SpMV(M.csr(S, p)) as op:
        got = S.block_sequence(op, U, V, length, trans=trans, d_left=d)
        again = S.block_sequence(op, U, V, length, trans=trans, d_left=d)
    assert got.tobytes() == want.tobytes()
    assert again.tobytes() == got.tobytes()


def test_sequence_on_device_tensors_and_its_refusals(S):
    import torch

    p, n, b, length = P16, 300, 4, 6
    rng = np.random.default_rng(5)
    M = short_rows_matrix(rng, n, p)
    U, V, d = rand_bal(rng, (n, b), p), rand_bal(rng, (n, b), p), rand_bal(rng, n, p)
    d[d == 0] = 1
    want = np_block_sequence(M, U, V, length, p, False, d)
    with S.SpMV(M.csr(S, p)) as op:
        tU, tV, td = (torch.from_numpy(a).cuda() for a in (U, V, d))
        got = S.block_sequence(op, tU, tV, length, d_left=td)
        assert got.device.type == "cuda" and got.cpu().numpy().tobytes() == want.tobytes()
        # a zero word of the diagonal, mod p
        for z in (0, p, -p):
            dz = d.copy()
            dz[3] = z
            with pytest.raises(S.SpasmError, match=r"spasm_amd_block_sequence: d_left\[3\] is zero mod p"):
                S.block_sequence(op, U, V, length, d_left=dz)
        with pytest.raises(S.SpasmError, match="b must be 2, 4, 8 or 16"):
            S.block_sequence(op, U[:, :3].copy(), V[:, :3].copy(), length)
        with pytest.raises(S.SpasmError, match=r"len out of range \(1 <= len < 2\^24\)"):
            S.block_sequence(op, U, V, 0)
        lib = S._abi.lib()
        out = np.full((length, b, b), 0x5A5A5A5A, dtype=np.int32)
        assert lib.spasm_amd_block_sequence(op._op, 0, b, length, None, None, b, V.ctypes.data, b, out.ctypes.data) == -1
        assert S._abi.last_error() == "spasm_amd_block_sequence: NULL array"
        assert lib.spasm_amd_block_sequence(op._op, 2, b, length, None, U.ctypes.data, b, V.ctypes.data, b, out.ctypes.data) == -1
        assert "bad arguments" in S._abi.last_error()
        assert lib.spasm_amd_block_sequence(op._op, 0, b, length, None, U.ctypes.data, b - 1, V.ctypes.data, b, out.ctypes.data) == -1
        assert "bad arguments" in S._abi.last_error()
        assert (out == 0x5A5A5A5A).all()
    tall = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)], []], 2, prime=127)
    with S.SpMV(tall) as op:
        with pytest.raises(S.SpasmError, match=r"not square \(3 x 2\)"):
            S.block_sequence(op, np.zeros((3, 2), dtype=np.int32), np.zeros((3, 2), dtype=np.int32), 4)


# ---------------------------------------------------------------- Berlekamp-Massey over matrix sequences
def to_lists(F):
    return [[[int(x) for x in row] for row in Ft] for Ft in F]


def check_generator(S, seq, b, p, hankel=True):
    """seq: (len, b, b) integers.  The reference confirms (C) alone: its degrees sum to the rank of the block Hankel matrix.  The
    device's F then has (A), (B) and the reference's degrees; two runs give the same bytes."""
    seq_l = [[[int(x) % p for x in row] for row in T] for T in seq]
    Fr, rdr = R.generator(seq_l, b, p)
    assert R.check_annihilates(Fr, rdr, seq_l, p) and R.check_row_reduced(Fr, rdr, p)
    if hankel:
        assert sum(rdr) == R.block_hankel_rank(seq_l, b, p)
    arr = bal(np.array(seq_l, dtype=object), p)
    F, rowdeg = S.block_berlekamp_massey(arr, p)
    F2, rowdeg2 = S.block_berlekamp_massey(arr, p)
    assert F.tobytes() == F2.tobytes() and rowdeg.tobytes() == rowdeg2.tobytes()
    assert F.dtype == np.int32 and F.shape == (int(rowdeg.max()) + 1, b, b)
    assert (np.abs(F.astype(np.int64)) <= p // 2).all()
    Fl, rd = to_lists(F), [int(x) for x in rowdeg]
    assert R.check_annihilates(Fl, rd, seq_l, p), "(A)"
    assert R.check_row_reduced(Fl, rd, p), "(B)"
    assert sorted(rd) == sorted(rdr), "(C)"
    st = S.block_stats()
    assert (st["b"], st["len"], st["degree_sum"], st["max_degree"]) == (b, len(seq_l), sum(rd), max(rd))
    return F, rd


@functools.lru_cache(maxsize=None)
def random_sequence(n, b, p):
    rng = np.random.default_rng(1000 * n + 10 * b + p % 7)
    M = short_rows_matrix(rng, n, p)
    U, V = rand_bal(rng, (n, b), p), rand_bal(rng, (n, b), p)
    return np_block_sequence(M, U, V, terms(n, b), p)


@pytest.mark.parametrize("b", WIDTHS)
@pytest.mark.parametrize("n", (1, 7, 64, 130))
@pytest.mark.parametrize("p", PRIMES3)
def test_generator_of_random_sequences(S, p, n, b):
    _, rd = check_generator(S, random_sequence(n, b, p), b, p)
    assert sum(rd) <= n


@pytest.mark.parametrize("b", WIDTHS)
@pytest.mark.parametrize("p", PRIMES3)
def test_generator_of_special_sequences(S, p, b):
    rng = np.random.default_rng(17 * b + p % 101)
    # the zero sequence: F = I, all degrees 0
    F, rd = check_generator(S, np.zeros((6, b, b), dtype=np.int64), b, p)
    assert rd == [0] * b and F.tolist() == [np.eye(b, dtype=np.int32).tolist()]
    # A = 0: S_0 = U^T V, then zeros
    n = 9
    Z = W.Mat.from_rows([[] for _ in range(n)], n)
    U, V = rand_bal(rng, (n, b), p), rand_bal(rng, (n, b), p)
    check_generator(S, np_block_sequence(Z, U, V, terms(n, b), p), b, p)
    # S_0 singular: two equal columns of U and a zero column of V
    n = 24
    M = short_rows_matrix(rng, n, p)
    U, V = rand_bal(rng, (n, b), p), rand_bal(rng, (n, b), p)
    U[:, 1] = U[:, 0]
    V[:, b - 1] = 0
    seq = np_block_sequence(M, U, V, terms(n, b) + 4, p)
    assert R.det_mod(seq[0].tolist(), p) == 0
    check_generator(S, seq, b, p)
    # a permutation matrix with many cycles: many invariant factors, the generator's degrees stay below n
    cycles, perm, at = (5, 5, 3, 3, 2, 2, 1, 1), [], 0
    for c in cycles:
        perm += [at + (k + 1) % c for k in range(c)]
        at += c
    n = at
    Pm = W.Mat(n, n, np.arange(n + 1), np.array(perm), np.ones(n, dtype=np.int64))
    U, V = rand_bal(rng, (n, b), p), rand_bal(rng, (n, b), p)
    _, rd = check_generator(S, np_block_sequence(Pm, U, V, 2 * n + 2, p), b, p)
    assert sum(rd) <= n


def test_a_long_sequence_spreads_the_discrepancy_over_workgroups(S):
    """len = 300 at b = 2: degrees up to 150, so the discrepancy takes three chunks of 64 coefficients and the update several
    workgroups; the sequence is that of a random sparse matrix of order 290"""
    p, n, b = P32, 290, 2
    seq = random_sequence(n, b, p)
    assert len(seq) == 292
    _, rd = check_generator(S, seq, b, p, hankel=False)
    assert max(rd) > 128


# ---------------------------------------------------------------- the determinant
def det_matrix(kind, n, p, seed):
    rng = np.random.default_rng(seed)
    if kind == "identity":
        return W.Mat(n, n, np.arange(n + 1), np.arange(n), np.ones(n, dtype=np.int64))
    D = np.zeros((n, n), dtype=np.int64)
    for i in range(n):
        cols = rng.choice(n, size=min(n, 5), replace=False)
        D[i, cols] = rng.integers(1, p, size=len(cols))
        D[i, i] = int(rng.integers(1, p))
    if kind == "singular":   # the last row is a combination of two others
        D[n - 1] = (D[0] * 2 + D[1] * 3) % p
    return W.Mat.from_dense(D)


def ref_det_tries(S, M, b, p, seed, tries):
    """the procedure of the header on the host: the generator's vectors and diagonal of each try, the numpy sequence, the
    reference's generator"""
    n = M.n
    for t in range(tries):
        U, V = S.minpoly_vectors(n, b, seed + t, p)
        d = S.precond_diagonal(n, seed + t, 0, p)
        seq = np_block_sequence(M, U, V, terms(n, b), p, False, d)
        seq_l = [[[int(x) % p for x in row] for row in T] for T in seq]
        F, rd = R.generator(seq_l, b, p)
        if sum(rd) != n:
            continue
        dlc = R.det_mod(R.leading_matrix(F, rd), p)
        prod = 1
        for x in d.tolist():
            prod = prod * (x % p) % p
        v = R.det_mod(F[0], p) * pow(dlc, p - 2, p) * pow(prod, p - 2, p) % p
        return (int(bal(np.array([-v if n & 1 else v], dtype=object), p)[0]), 1)
    return (0, 0)


DET_CASES = [("random", 5, 2), ("random", 64, 8), ("random", 181, 8), ("random", 300, 16), ("random", 64, 4), ("singular", 60, 4),
             ("identity", 40, 8)]


@pytest.mark.parametrize("kind,n,b", DET_CASES)
@pytest.mark.parametrize("p", (P16, P32))
def test_determinant_at_the_large_primes(S, p, kind, n, b):
    M = det_matrix(kind, n, p, 100 + n)
    A = M.csr(S, p)
    want = S.det(A)
    det, status = S.block_wiedemann_det(A, b=b, seed=1, tries=3)
    assert status == 1   # (the seeds were run through the reference on the host: it fails on none of these)
    assert det == want
    assert (kind == "singular") == (det == 0)
    st = S.block_stats()
    assert st["steps"] == terms(n, b) - 1 <= 2 * -(-n // b) + 2 and st["len"] == terms(n, b)   # the sequence really is short
    assert st["tries"] == 1 and st["degree_sum"] == n and st["b"] == b and st["n"] == n
    # the three entries agree, and two runs give the same answer
    with S.SpMV(A) as op:
        assert op.block_wiedemann_det(b=b, seed=1, tries=3) == (det, status)
    Dm = S.DeviceCSR(A)
    assert Dm.block_wiedemann_det(b=b, seed=1, tries=3) == (det, status)
    assert S.block_wiedemann_det(A, b=b, seed=1, tries=3) == (det, status)


@pytest.mark.parametrize("kind,n,b", [("random", 5, 2), ("random", 64, 8), ("random", 30, 4), ("singular", 24, 2), ("identity", 2, 2)])
def test_determinant_over_gf3_fails_at_most_where_the_reference_fails(S, kind, n, b):
    p = P3
    M = det_matrix(kind, n, p, 300 + n)
    A = M.csr(S, p)
    got = S.block_wiedemann_det(A, b=b, seed=2, tries=3)
    ref = ref_det_tries(S, M, b, p, 2, 3)
    assert got == ref
    if got[1] == 1:
        assert got[0] == S.det(A)
