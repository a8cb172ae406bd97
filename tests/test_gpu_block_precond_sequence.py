"""GPU tests of spasm_amd_block_precond_sequence: the block sequence of the composite operator
M = diag(d_right) op(A)^T diag(d_left) op(A) (two launch sets a step: csrc/precond.hpp's DiagEpi on one view, csrc/block_krylov.hpp's
BlockEpi on the other), byte for byte against exact numpy int64 products, for square and rectangular matrices in both
orientations, and against spasm_amd_precond_sequence column by column."""
import numpy as np
import pytest

import nullspace_cases as K
import wiedemann_ref as W
from nullspace_cases import P3, P16, P32
from test_gpu_block_wiedemann import long_row_matrix, short_rows_matrix
from wiedemann_ref import bal

pytestmark = pytest.mark.gpu

PRIMES3 = (P3, P16, P32)


def raw(rng, shape):
    """unreduced int32 words, the extremes among them"""
    a = rng.integers(-2**31, 2**31, size=shape, dtype=np.int64).astype(np.int32)
    a.flat[0], a.flat[-1] = 2**31 - 1, -2**31
    return a


def check(S, M, op, p, b, trans, with_right, rng, length):
    B = M.transpose() if trans else M
    nr, dim = B.n, B.m
    U, V = raw(rng, (dim, b)), raw(rng, (dim, b))
    dl = raw(rng, nr)
    dr = raw(rng, dim) if with_right else None
    U0, V0 = U.copy(), V.copy()
    got = S.block_precond_sequence(op, U, V, length, dl, dr, trans=trans)
    assert got.shape == (length, b, b) and got.dtype == np.int32
    want = bal(K.np_block_precond_sequence(B, U, V, length, dl, dr, p), p)
    assert got.tobytes() == want.tobytes()
    assert op.block_precond_sequence(U, V, length, dl, dr, trans=trans).tobytes() == got.tobytes()   # two runs
    assert U.tobytes() == U0.tobytes() and V.tobytes() == V0.tobytes()
    st = S.wiedemann_kernel_stats()
    assert (st["b"], st["sequence_products"], st["products"]) == (b, 2 * (length - 1), 2 * (length - 1))
    return got


@pytest.mark.parametrize("with_right", (False, True))
@pytest.mark.parametrize("trans", (False, True))
@pytest.mark.parametrize("b", (2, 4, 8, 16))
@pytest.mark.parametrize("p", PRIMES3)
def test_the_composite_sequence_on_short_rows_square_and_rectangular(S, p, b, trans, with_right):
    rng = np.random.default_rng(17 * b + p % 1009 + 2 * int(trans) + int(with_right))
    mats = [short_rows_matrix(rng, 70, p, empty=True)]
    for n, m in ((20, 33), (40, 30)):
        D = np.where(rng.random((n, m)) < 0.2, rng.integers(1, p, size=(n, m)), 0)
        mats.append(W.Mat.from_dense(D))
    for M in mats:
        with S.SpMV(M.csr(S, p)) as op:
            check(S, M, op, p, b, trans, with_right, rng, 5)
            check(S, M, op, p, b, trans, with_right, rng, 1)


@pytest.mark.parametrize("trans", (False, True))
@pytest.mark.parametrize("b", (2, 16))
@pytest.mark.parametrize("p", PRIMES3)
def test_the_composite_sequence_on_the_long_row(S, p, b, trans):
    rng = np.random.default_rng(23 * b + p % 1009 + int(trans))
    M = long_row_matrix(rng, 16500, p)
    with S.SpMV(M.csr(S, p)) as op:
        check(S, M, op, p, b, trans, True, rng, 4)


@pytest.mark.parametrize("p", PRIMES3)
def test_the_diagonal_of_the_block_is_precond_sequence_mode_1(S, p):
    """b = 2, U's and V's columns one by one: S[i, c, c] is the scalar sequence of E A^T D2 A on (U[:, c], V[:, c])"""
    rng = np.random.default_rng(p % 1009)
    n, m, length = 40, 30, 6
    D = np.where(rng.random((n, m)) < 0.2, rng.integers(1, p, size=(n, m)), 0)
    M = W.Mat.from_dense(D)
    U, V = raw(rng, (m, 2)), raw(rng, (m, 2))
    dl, dr = raw(rng, n), raw(rng, m)
    with S.SpMV(M.csr(S, p)) as op:
        blk = S.block_precond_sequence(op, U, V, length, dl, dr)
        sc = S.precond_sequence(op, 1, dl, dr, U, V, length)
        for c in range(2):
            one = S.precond_sequence(op, 1, dl, dr, np.ascontiguousarray(U[:, c:c + 1]), np.ascontiguousarray(V[:, c:c + 1]), length)
            assert blk[:, c, c].tobytes() == one[:, 0].tobytes() == np.ascontiguousarray(sc[:, c]).tobytes()


def test_the_refusals_that_need_an_operator(S):
    p = P16
    M = W.Mat.from_dense(np.array([[1, 2, 0], [0, 3, 4]]))
    err = S._abi.last_error
    lib = S._abi.lib()
    who = "spasm_amd_block_precond_sequence"
    a = np.ones((3, 16), dtype=np.int32)
    d = np.ones(3, dtype=np.int32)
    out = np.full(4096, 0x5A5A5A5A, dtype=np.int32)
    ptr = lambda x: x.ctypes.data
    with S.SpMV(M.csr(S, p)) as op:
        call = lambda b, ln, dl, dr, U, ldu, V, ldv, S_, tr=0: lib.spasm_amd_block_precond_sequence(op._op, tr, b, ln, dl, dr, U, ldu, V, ldv, S_)
        assert call(3, 2, ptr(d), None, ptr(a), 16, ptr(a), 16, ptr(out)) == -1 and err() == f"{who}: b must be 2, 4, 8 or 16"
        for ln in (0, -1, 2**24):
            assert call(2, ln, ptr(d), None, ptr(a), 16, ptr(a), 16, ptr(out)) == -1 and err() == f"{who}: len out of range (1 <= len < 2^24)"
        for args in ((1, 16, 0), (16, 1, 0), (16, 16, 2)):
            assert call(2, 2, ptr(d), None, ptr(a), args[0], ptr(a), args[1], ptr(out), args[2]) == -1
            assert err() == f"{who}: bad arguments (trans 0/1, ldu >= b, ldv >= b)"
        assert call(2, 2, None, None, ptr(a), 16, ptr(a), 16, ptr(out)) == -1 and err() == f"{who}: NULL array"
        assert call(2, 2, ptr(d), None, None, 16, ptr(a), 16, ptr(out)) == -1 and err() == f"{who}: NULL array"
        assert call(2, 2, ptr(d), None, ptr(a), 16, ptr(a), 16, None) == -1 and err() == f"{who}: NULL array"
        assert (out == 0x5A5A5A5A).all()
        with pytest.raises(ValueError):
            S.block_precond_sequence(op, np.ones((2, 2), dtype=np.int32), np.ones((2, 2), dtype=np.int32), 2, d[:2])   # dim is 3


@pytest.mark.parametrize("p", PRIMES3)
def test_an_operator_without_rows_or_columns_takes_the_host_path(S, p):
    """op(A) of 0 rows or 0 columns: M = 0, so S_0 = U^T V and every later term is zero (computed on the host)"""
    rng = np.random.default_rng(p % 1009 + 5)
    b, length = 4, 3
    for rows, cols in ((0, 3), (3, 0)):
        M = W.Mat.from_rows([[] for _ in range(rows)], cols)
        with S.SpMV(M.csr(S, p)) as op:
            for trans in (False, True):
                nr, dim = (cols, rows) if trans else (rows, cols)
                U, V = raw(rng, (dim, b)) if dim else np.zeros((0, b), dtype=np.int32), rand_block(rng, dim, b)
                dl = np.ones(nr, dtype=np.int32)
                got = S.block_precond_sequence(op, U, V, length, dl, trans=trans)
                want = np.zeros((length, b, b), dtype=np.int64)
                want[0] = np.array([[sum(int(U[k, r]) * int(V[k, c]) for k in range(dim)) % p for c in range(b)] for r in range(b)])
                assert got.tobytes() == bal(want, p).tobytes(), (rows, cols, trans)


def rand_block(rng, dim, b):
    return rng.integers(-2**31, 2**31, size=(dim, b), dtype=np.int64).astype(np.int32)
