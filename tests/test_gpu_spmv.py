"""Exact products y <- A x + y and y <- x A + y on the device (spasm_Axpy, spasm_xApy, the resident operator spasm_amd_spmv_*,
CSR @ and SpMV).  Every expected value comes from exact integer numpy: products reduced per entry, then np.add.at."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PRIMES = [3, 127, 42013, 65521, 2**31 - 1, 0xFFFFFFFB]


def csr_arrays(A):
    k = int(A.p[A.n])
    return np.asarray(A.p, dtype=np.int64).copy(), A.j[:k].astype(np.int64), A.x[:k].astype(np.int64)


def ref(A, X, Y, trans):
    """Y + op(A) X mod p as balanced residues, with exact integers: X of shape (rows_in, k), Y of shape (rows_out, k)"""
    p = A.prime
    ptr, j, v = csr_arrays(A)
    row = np.repeat(np.arange(A.n), np.diff(ptr))
    src, dst = (row, j) if trans else (j, row)
    X = np.asarray(X, dtype=np.int64) % p
    acc = np.asarray(Y, dtype=np.int64) % p
    prod = ((v % p).astype(np.uint64)[:, None] * X[src].astype(np.uint64)) % np.uint64(p)  # < p^2 < 2^64
    np.add.at(acc, dst, prod.astype(np.int64))  # nnz * p < 2^63
    acc %= p
    return np.where(2 * acc > p, acc - p, acc).astype(np.int32)


def rand_csr(S, n, m, density, p, rng, empty_every=0):
    """n x m with balanced values, columns unsorted inside rows, every empty_every-th row empty"""
    rows = []
    for i in range(n):
        cnt = 0 if (empty_every and i % empty_every == 0) else rng.binomial(m, density)
        cols = rng.choice(m, size=cnt, replace=False) if cnt else np.zeros(0, dtype=np.int64)
        rows.append(cols)
    ptr = np.zeros(n + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    j = np.concatenate(rows).astype(np.int32) if n else np.zeros(0, np.int32)
    vals = rng.integers(1, p, size=len(j), dtype=np.int64)
    x = S.balanced(vals, p)
    return S.CSR.from_arrays(n, m, ptr, j, x, prime=p)


def rand_int32(rng, shape):
    return rng.integers(-(2**31), 2**31, size=shape, dtype=np.int64).astype(np.int32)


def test_readme_kernel_vector(S):
    sm = S.CSR(np.array([[1, 2], [3, 6]]))
    assert (sm @ np.array([3, -1])).tolist() == [0, 0]
    assert (sm @ [3, 42012]).tolist() == [0, 0]


@pytest.mark.parametrize("p", PRIMES)
@pytest.mark.parametrize("shape", [(40, 40), (17, 300), (300, 17), (0, 9), (9, 0), (0, 0)])
def test_one_shot_products_exact(S, p, shape):
    rng = np.random.default_rng(p + 7 * shape[0] + shape[1])
    n, m = shape
    A = rand_csr(S, n, m, 0.2, p, rng, empty_every=5)
    for trans in (False, True):
        rin, rout = (n, m) if trans else (m, n)
        x = rand_int32(rng, rin)  # unreduced inputs in x and y
        y = rand_int32(rng, rout)
        want = ref(A, x[:, None], y[:, None], trans)[:, 0]
        got = y.copy()
        (S.xapy(x, A, got) if trans else S.axpy(A, x, got))
        assert np.array_equal(got, want), (p, shape, trans)
        # reduced inputs, y = 0 through the operators
        xr = S.balanced(x, p)
        z = np.zeros(rout, dtype=np.int32)
        assert np.array_equal(xr @ A if trans else A @ xr, ref(A, xr[:, None], z[:, None], trans)[:, 0])


@pytest.mark.parametrize("p", [127, 65521, 0xFFFFFFFB])
def test_blocks_equal_single_products(S, p):
    rng = np.random.default_rng(p)
    n, m = 90, 70
    A = rand_csr(S, n, m, 0.1, p, rng, empty_every=7)
    with S.SpMV(A) as op:
        for k in (1, 2, 3, 8, 31, 64, 100):
            for trans in (False, True):
                rin, rout = (n, m) if trans else (m, n)
                X = rand_int32(rng, (rin, k))
                Ybig = rand_int32(rng, (rout, k + 5))  # leading dimension k + 5
                Y = Ybig[:, 2:2 + k]
                Y0, Ybig0 = Y.copy(), Ybig.copy()
                op.apply(X, Y, trans=trans)
                for c in range(k):
                    y = Y0[:, c].copy()
                    (S.xapy(np.ascontiguousarray(X[:, c]), A, y) if trans else S.axpy(A, np.ascontiguousarray(X[:, c]), y))
                    assert np.array_equal(Y[:, c], y), (k, trans, c)
                assert np.array_equal(Y, ref(A, X, Y0, trans))
                assert np.array_equal(Ybig[:, :2], Ybig0[:, :2]) and np.array_equal(Ybig[:, k + 2:], Ybig0[:, k + 2:])
        # the (k, n) @ A and A @ (m, k) forms
        Xr = rng.integers(0, p, size=(5, n))
        assert np.array_equal(Xr @ A, ref(A, Xr.T, np.zeros((m, 5), np.int32), True).T)
        Xc = rng.integers(0, p, size=(m, 6))
        assert np.array_equal(A @ Xc, ref(A, Xc, np.zeros((n, 6), np.int32), False))


@pytest.mark.parametrize("p", [65521, 0xFFFFFFFB])
def test_accumulator_bounds_long_row_and_column(S, p):
    """4 194 304 terms of halfp * halfp into one output: the long-row segments and their exact combination, in both orientations"""
    L = 4_194_304
    h = p // 2
    want = S.ZZp(p, L * h * h)
    row = S.CSR.from_arrays(1, L, np.array([0, L]), np.arange(L, dtype=np.int32), np.full(L, h, dtype=np.int32), prime=p)
    x = np.full(L, h, dtype=np.int32)
    y = np.zeros(1, dtype=np.int32)
    assert S.axpy(row, x, y)[0] == want
    col = S.CSR.from_arrays(L, 1, np.arange(L + 1), np.zeros(L, dtype=np.int32), np.full(L, h, dtype=np.int32), prime=p)
    y = np.zeros(1, dtype=np.int32)
    assert S.xapy(x, col, y)[0] == want
    # the other orientation of each: L outputs of one term each
    assert np.array_equal(S.axpy(col, np.array([h], np.int32), np.zeros(L, np.int32)), np.full(L, S.ZZp(p, h * h), np.int32))
    assert np.array_equal(S.xapy(np.array([h], np.int32), row, np.zeros(L, np.int32)), np.full(L, S.ZZp(p, h * h), np.int32))


def test_operator_outlives_host_matrix_and_torch_path(S):
    import torch

    p = 42013
    rng = np.random.default_rng(5)
    n, m = 500, 400
    A = rand_csr(S, n, m, 0.02, p, rng, empty_every=11)
    ptr, j, v = csr_arrays(A)
    op = S.SpMV(A)
    del A
    gc.collect()
    B = S.CSR.from_arrays(n, m, ptr, j.astype(np.int32), v.astype(np.int32), prime=p)  # the same matrix, for the one-shot calls
    try:
        for t in range(10):
            k = [1, 2, 5, 8, 16, 33, 64, 3, 7, 100][t]
            for trans in (False, True):
                rin, rout = (n, m) if trans else (m, n)
                X = rand_int32(rng, (rin, k))
                Y0 = rand_int32(rng, (rout, k))
                Y = op.apply(X, Y0.copy(), trans=trans)
                for c in range(0, k, max(1, k // 4)):
                    y = Y0[:, c].copy()
                    (S.xapy(np.ascontiguousarray(X[:, c]), B, y) if trans else S.axpy(B, np.ascontiguousarray(X[:, c]), y))
                    assert np.array_equal(Y[:, c], y)
                Xt = torch.from_numpy(X).cuda()
                Yt = torch.from_numpy(Y0).cuda()
                assert op.apply(Xt, Yt, trans=trans) is Yt
                torch.cuda.synchronize()
                assert np.array_equal(Yt.cpu().numpy(), Y)
                v1 = op.apply(torch.from_numpy(np.ascontiguousarray(X[:, 0])).cuda(), trans=trans)
                assert np.array_equal(v1.cpu().numpy(), ref(B, X[:, :1], np.zeros((rout, 1), np.int32), trans)[:, 0])
    finally:
        op.close()
    with pytest.raises(S.SpasmError):
        op.apply(np.zeros(m, np.int32))


def test_config3_full_size_exact(S):
    A = S.synth_csr(1, 1_000_000, 1_000_000, row_nnz=20, prime=65521, seed=0x5A5A0003)
    rng = np.random.default_rng(3)
    x = S.balanced(rng.integers(0, 65521, size=A.m), 65521)
    assert np.array_equal(A @ x, ref(A, x[:, None], np.zeros((A.n, 1), np.int32), False)[:, 0])
    w = S.balanced(rng.integers(0, 65521, size=A.n), 65521)
    assert np.array_equal(w @ A, ref(A, w[:, None], np.zeros((A.m, 1), np.int32), True)[:, 0])


def test_kernel_basis_through_operator(S):
    """10k x 10k, density 1e-3, its last 150 rows empty so that the kernel has at least 150 vectors with many entries"""
    p = 42013
    B = S.synth_csr(0, 9_850, 10_000, density=1e-3, prime=p, seed=0x5A5A0007)
    ptr, j, v = csr_arrays(B)
    A = S.CSR.from_arrays(10_000, 10_000, np.concatenate([ptr, np.full(150, ptr[-1])]), j.astype(np.int32), v.astype(np.int32), prime=p)
    K = S.kernel(S.echelonize(A))
    assert K.n >= 150 and K.m == A.m
    Kt = K.todense().T.astype(np.int32).copy()  # m x dim(ker)
    with S.SpMV(A) as op:
        got = op.apply(Kt)
    assert not got.any()
    assert not ref(A, Kt, np.zeros((A.n, K.n), np.int32), False).any()
