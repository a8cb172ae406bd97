"""GPU tests of the characteristic-polynomial entries (spasm_amd_charpoly_batch / _charpoly / _dcsr_charpoly; csrc/charpoly.hpp).

chi_A(x) = det(x * I - A), monic, n + 1 balanced residues, low degree first.  Two references are written here and checked against
each other: the division-free Berkowitz algorithm in Python integers (n <= 20), and the Hessenberg reduction with the recurrence
over the leading principal minors in numpy int64 (products of two residues of a prime above 2^31 are taken in two 16-bit halves of
one factor, so every intermediate stays below 2^49).  Where stated the polynomial is known by construction instead: companion
matrices and what is similar to them, triangular matrices, the shift, the identity, block-diagonal matrices."""
import ctypes as C
from math import comb

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P16, P31, P32 = 65521, 2147483647, 4294967291
PRIMES = (3, 5, 127, P16, P31, P32)
SENTINEL = 0x5A5A5A5A


# ---------------------------------------------------------------------------------------------
# the references and the constructions
# ---------------------------------------------------------------------------------------------
def bal(v, p):
    """integers -> the int32 array of their balanced residues"""
    v = np.array([int(x) % p for x in np.asarray(v, dtype=object).ravel()], dtype=np.int64)
    return np.where(v > p // 2, v - p, v).astype(np.int32)


def mulmod(a, b, p):
    """a * b mod p for int64 arrays of residues in [0, p), p < 2^32"""
    if p < 2**31:
        return a * b % p
    return ((a * (b >> 16) % p) * 65536 + a * (b & 0xFFFF)) % p


def berkowitz(D, p):
    """chi of the integer matrix D mod p, low degree first, residues in [0, p): no division at all"""
    n = len(D)
    A = [[int(v) % p for v in row] for row in D]
    vec = [1]   # high degree first
    for r in range(n):
        a, R, Cc = A[r][r], A[r][:r], [A[i][r] for i in range(r)]
        col = [1, -a % p]   # the first column of the Toeplitz factor: 1, -a, -R C, -R M C, -R M^2 C, ...
        v = Cc
        for _ in range(r):
            col.append(-sum(x * y for x, y in zip(R, v)) % p)
            v = [sum(A[i][j] * v[j] for j in range(r)) % p for i in range(r)]
        vec = [sum(col[i - j] * vec[j] for j in range(len(vec)) if 0 <= i - j < len(col)) % p for i in range(r + 2)]
    return vec[::-1]


def host_charpoly(D, p, pivots=None):
    """chi of the integer matrix D mod p by Hessenberg reduction and the recurrence, low degree first, residues in [0, p); the
    pivot row of every step that has one is appended to `pivots` as (k, row)"""
    M = np.array(D, dtype=np.int64).reshape(len(D), len(D)) % p
    n = len(M)
    for k in range(n - 2):
        nz = np.nonzero(M[k + 1:, k])[0]
        if len(nz) == 0:
            continue
        pr = k + 1 + int(nz[0])
        if pivots is not None:
            pivots.append((k, pr))
        if pr != k + 1:
            M[[k + 1, pr]] = M[[pr, k + 1]]
            M[:, [k + 1, pr]] = M[:, [pr, k + 1]]
        f = mulmod(M[k + 2:, k], np.int64(pow(int(M[k + 1, k]), -1, p)), p)
        M[k + 2:] = (M[k + 2:] - mulmod(f[:, None], M[k + 1][None, :], p)) % p
        M[:, k + 1] = (M[:, k + 1] + mulmod(M[:, k + 2:], f[None, :], p).sum(axis=1)) % p
    pol = np.zeros((n + 1, n + 2), dtype=np.int64)   # pol[i, j] = coefficient j of p_i
    pol[0, 0] = 1
    t = np.ones(n, dtype=np.int64)   # t[i] = h_{i+1,i} * ... * h_{k,k-1}
    for k in range(n):
        if k > 0:
            t[:k] = mulmod(t[:k], M[k, k - 1], p)
        c = mulmod(M[: k + 1, k], t[: k + 1], p)   # (t[k] = 1: the term of h_kk)
        pol[k + 1, 1:] = pol[k, :-1]
        pol[k + 1] = (pol[k + 1] - mulmod(c[:, None], pol[: k + 1], p).sum(axis=0)) % p
    return [int(v) for v in pol[n, : n + 1]]


def polymul(a, b, p):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + int(x) * int(y)) % p
    return out


def csr_raw(S, D, p):
    """the CSR of the dense integer matrix D with its non-zero entries AS THEY ARE (no reduction on the host)"""
    D = np.asarray(D, dtype=np.int64).reshape(len(D), -1 if len(D) else 0)
    n = D.shape[0]
    rows, cols = np.nonzero(D)
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ptr[1:])
    return S.CSR.from_arrays(n, n, ptr, cols, D[rows, cols], prime=p)


def csr_of(S, D, p):
    """the CSR of D mod p, balanced"""
    D = np.asarray(D, dtype=np.int64) % p
    return csr_raw(S, np.where(D > p // 2, D - p, D), p)


def random_dense(rng, n, p):
    return rng.integers(0, p, size=(n, n), dtype=np.int64)


def random_sparse(rng, n, p, per_row=4):
    D = np.zeros((n, n), dtype=np.int64)
    for i in range(n):
        D[i, rng.integers(0, n, size=per_row)] = rng.integers(1, p, size=per_row)
    return D


def companion(coef, p):
    """the companion matrix of the monic polynomial coef (low degree first, coef[n] = 1): ones on the subdiagonal, -coef in the
    last column; its characteristic polynomial is coef"""
    n = len(coef) - 1
    D = np.zeros((n, n), dtype=np.int64)
    D[np.arange(1, n), np.arange(n - 1)] = 1
    D[:, n - 1] = [-int(c) % p for c in coef[:n]]
    return D


def random_monic(rng, n, p):
    return [int(v) for v in rng.integers(0, p, size=n)] + [1]


def unit_lower_inverse(L, p):
    """the inverse mod p of a unit lower triangular matrix, p < 2^31"""
    n = len(L)
    inv = np.eye(n, dtype=np.int64)
    for i in range(1, n):
        inv[i, :i] = -(L[i, :i] @ inv[:i, :i]) % p
    return inv


def check(got, want, p):
    want = bal(want, p)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]


# ---------------------------------------------------------------------------------------------
# the references agree with each other (and with sympy on a tiny case)
# ---------------------------------------------------------------------------------------------
def test_references_agree_with_each_other():
    rng = np.random.default_rng(0xC4A0)
    for p in (3, 5, 127, P16, P32):
        for n in (0, 1, 2, 3, 7, 20):
            for D in (random_dense(rng, n, p), random_sparse(rng, n, p, 2) if n else np.zeros((0, 0), dtype=np.int64)):
                assert berkowitz(D, p) == host_charpoly(D, p), (p, n)
    try:
        import sympy
    except ImportError:   # the two references above do not need it
        return
    D = [[2, -1, 0, 5], [7, 3, 1, 0], [0, 4, -6, 2], [1, 0, 9, 8]]
    x = sympy.symbols("x")
    want = [int(c) % 127 for c in sympy.Matrix(D).charpoly(x).all_coeffs()[::-1]]
    assert berkowitz(D, 127) == want and host_charpoly(D, 127) == want


# ---------------------------------------------------------------------------------------------
# tiny and unreduced input
# ---------------------------------------------------------------------------------------------
def test_tiny_matrices(S):
    p = 127
    out = S.charpoly_batch([csr_raw(S, np.zeros((0, 0)), p), csr_raw(S, [[5]], p), csr_raw(S, [[0]], p), csr_raw(S, [[1, 2], [3, 4]], p),
                            csr_raw(S, [[0, 1, 0], [0, 0, 1], [2, 3, 4]], p)])
    check(out[0], [1], p)
    check(out[1], [-5, 1], p)
    check(out[2], [0, 1], p)
    check(out[3], [-2, -5, 1], p)
    check(out[4], [-2, -3, -4, 1], p)   # the transposed companion matrix of x^3 - 4 x^2 - 3 x - 2
    check(S.charpoly(csr_raw(S, np.zeros((0, 0)), P32)), [1], P32)


def test_entries_outside_the_balanced_range_and_negative_entries_are_reduced(S):
    rng = np.random.default_rng(0xC4A1)
    for p in (5, 127, P16, P32):
        D = rng.integers(-2**31, 2**31, size=(9, 9), dtype=np.int64)
        D[0, 0], D[1, 1], D[2, 2] = 2**31 - 1, -2**31, p if p < 2**31 else -7
        D[3, 4] = 0
        want = berkowitz(D, p)
        assert want == host_charpoly(D, p)
        check(S.charpoly(csr_raw(S, D, p)), want, p)


# ---------------------------------------------------------------------------------------------
# known by construction: companion matrices, on both sides of every class boundary
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 31, 32, 33, 63, 64, 65, 110, 111, 181])
def test_companion_matrices_and_their_conjugates(S, n):
    p = P16
    rng = np.random.default_rng(0xC0 + n)
    coef = random_monic(rng, n, p)
    Cm = companion(coef, p)
    A = csr_of(S, Cm, p)
    # as it is: Hessenberg already, every pivot on the subdiagonal
    check(S.charpoly(A), coef, p)
    # conjugated by a random permutation, on the device
    perm = rng.permutation(n)
    with S.DeviceCSR(A) as dA, dA.permute(perm, perm) as dB:
        check(dB.charpoly(), coef, p)
        assert dB.download().equals(csr_of(S, Cm[np.ix_(perm, perm)], p))
    # conjugated by T = P * L1 * U1: a dense similar matrix, multiplied out by the device's products
    L = np.tril(rng.integers(0, p, size=(n, n), dtype=np.int64), -1) + np.eye(n, dtype=np.int64)
    U = np.triu(rng.integers(0, p, size=(n, n), dtype=np.int64), 1) + np.eye(n, dtype=np.int64)
    Li, Ui = unit_lower_inverse(L, p), unit_lower_inverse(U.T.copy(), p).T
    assert np.array_equal(L @ Li % p, np.eye(n, dtype=np.int64)) and np.array_equal(U @ Ui % p, np.eye(n, dtype=np.int64))
    Pm = np.eye(n, dtype=np.int64)[rng.permutation(n)]
    T, Ti = csr_of(S, Pm @ L % p @ U % p, p), csr_of(S, Ui @ Li % p @ Pm.T % p, p)
    B = (T @ A) @ Ti
    assert S.nnz(B) > n * n // 2 or n < 4
    check(S.charpoly(B), coef, p)


def test_companion_matrix_on_the_global_path_beyond_the_first_block_of_rows(S):
    p, n = P32, 600
    rng = np.random.default_rng(0xC600)
    coef = random_monic(rng, n, p)
    A = csr_of(S, companion(coef, p), p)
    check(S.charpoly(A), coef, p)
    assert S.charpoly_stats()["global_path"] == 1 and S.charpoly_stats()["lds_path"] == 0
    perm = rng.permutation(n)
    with S.DeviceCSR(A) as dA, dA.permute(perm, perm) as dB:
        check(dB.charpoly(), coef, p)


# ---------------------------------------------------------------------------------------------
# the pivot search
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", [(20, 127), (31, P32), (63, P16), (100, P32), (181, P16), (182, P32), (530, P16)])
def test_pivot_in_the_last_row(S, n, p):
    """the only non-zero below the diagonal of column k0 sits in the LAST row, and the columns left of k0 have nothing there (their
    steps are skipped): beyond the first wave for n > 64, beyond the first block of 512 rows for n = 530; the later columns fill in
    as the swap and the column operations go on"""
    rng = np.random.default_rng(0xC700 + n)
    for k0 in (0, 3):
        D = np.triu(random_sparse(rng, n, p, 6 if n < 200 else 3), -1)
        for c in range(k0 + 1):
            D[c + 1:, c] = 0
        D[n - 1, k0] = int(rng.integers(1, p))
        pivots = []
        want = host_charpoly(D, p, pivots)
        assert pivots[0] == (k0, n - 1)
        if n <= 20:
            assert want == berkowitz(D, p)
        check(S.charpoly(csr_of(S, D, p)), want, p)


def test_columns_without_anything_below_the_subdiagonal_are_skipped(S):
    rng = np.random.default_rng(0xC701)
    for n, p in ((40, 5), (100, P32)):
        # upper triangular: every step is skipped and chi is the product of the x - d_i
        D = np.triu(random_dense(rng, n, p))
        want = [1]
        for i in range(n):
            want = polymul(want, [-int(D[i, i]) % p, 1], p)
        check(S.charpoly(csr_of(S, D, p)), want, p)
        # every other column skipped
        D = np.triu(random_dense(rng, n, p), -1)
        D[np.arange(1, n, 2), np.arange(0, n - 1, 2)] = 0
        D[n - 1, 2] = 1
        check(S.charpoly(csr_of(S, D, p)), host_charpoly(D, p), p)


def test_shift_identity_and_block_diagonal(S):
    rng = np.random.default_rng(0xC702)
    for n, p in ((33, 3), (150, P32)):
        shift = np.zeros((n, n), dtype=np.int64)
        shift[np.arange(n - 1), np.arange(1, n)] = 1
        check(S.charpoly(csr_of(S, shift, p)), [0] * n + [1], p)
        check(S.charpoly(csr_of(S, shift.T, p)), [0] * n + [1], p)
        check(S.charpoly(csr_of(S, np.eye(n, dtype=np.int64), p)), [comb(n, k) * (-1) ** (n - k) for k in range(n + 1)], p)
    p = P16
    sizes = (7, 1, 20, 33, 12)
    blocks = [random_dense(rng, b, p) for b in sizes]
    n = sum(sizes)
    D = np.zeros((n, n), dtype=np.int64)
    at, want = 0, [1]
    for Bk in blocks:
        D[at:at + len(Bk), at:at + len(Bk)] = Bk
        at += len(Bk)
        want = polymul(want, berkowitz(Bk, p), p)
    check(S.charpoly(csr_of(S, D, p)), want, p)
    perm = rng.permutation(n)
    check(S.charpoly(csr_of(S, D[np.ix_(perm, perm)], p)), want, p)


# ---------------------------------------------------------------------------------------------
# primes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PRIMES)
def test_every_prime_with_n_above_small_primes(S, p):
    rng = np.random.default_rng(0xC800 + p % 1000)
    mats = [random_dense(rng, 20, p), random_sparse(rng, 20, p, 3), random_dense(rng, 45, p)]
    want = [host_charpoly(D, p) for D in mats]
    assert want[0] == berkowitz(mats[0], p) and want[1] == berkowitz(mats[1], p)
    for got, w in zip(S.charpoly_batch([csr_of(S, D, p) for D in mats]), want):
        check(got, w, p)


@pytest.mark.parametrize("n", [32, 181])
def test_entries_of_largest_magnitude_everywhere(S, n):
    """every entry is +(p - 1) / 2 or -(p - 1) / 2: the largest products the arithmetic meets (no lazy accumulator is used: every
    term is reduced by zp_axpy, whose double quotient must hold at |a * x + y| <= (p - 1)^2 / 4 + (p - 1) / 2)"""
    rng = np.random.default_rng(0xC900 + n)
    mats, want = [], []
    for p in PRIMES:
        h = (p - 1) // 2
        D = np.where(rng.integers(0, 2, size=(n, n)) == 1, h, -h).astype(np.int64)
        mats.append(csr_raw(S, D, p))
        assert int(np.abs(mats[-1].x[: n * n]).min()) == h
        want.append(host_charpoly(D, p))
    for got, w, p in zip(S.charpoly_batch(mats), want, PRIMES):
        check(got, w, p)


# ---------------------------------------------------------------------------------------------
# cross-checks against the rest of the engine
# ---------------------------------------------------------------------------------------------
def test_constant_term_is_the_determinant_and_second_coefficient_the_trace(S):
    rng = np.random.default_rng(0xCA00)
    mats, dense, primes = [], [], []
    for n, p in ((1, 127), (2, P16), (9, 3), (24, P32), (31, P16), (64, P31), (65, P32), (120, 127), (181, P32)):
        D = random_dense(rng, n, p) if n != 120 else random_sparse(rng, n, p, 5)
        dense.append(D)
        primes.append(p)
        mats.append(csr_of(S, D, p))
    dets = S.det_batch(mats).tolist()
    for c, D, p, d in zip(S.charpoly_batch(mats), dense, primes, dets):
        n = len(D)
        assert int(c[n]) == 1
        assert int(c[0]) == int(bal([(-1) ** n * d], p)[0]), (n, p)
        assert int(c[n - 1]) == int(bal([-sum(int(D[i, i]) for i in range(n))], p)[0]), (n, p)


def test_transpose_and_products_in_either_order(S):
    rng = np.random.default_rng(0xCA01)
    for n, p in ((17, 5), (50, P16), (90, P32)):
        A, B = csr_of(S, random_sparse(rng, n, p, 4), p), csr_of(S, random_sparse(rng, n, p, 3), p)
        ca = S.charpoly(A)
        assert np.array_equal(ca, S.charpoly(S.transpose(A)))
        with S.DeviceCSR(A) as dA, dA.transpose() as dT:
            assert np.array_equal(ca, dT.charpoly())
        assert np.array_equal(S.charpoly(A @ B), S.charpoly(B @ A))


@pytest.mark.parametrize("n,p", [(5, 3), (12, P16), (24, P32)])
def test_cayley_hamilton(S, n, p):
    rng = np.random.default_rng(0xCA02 + n)
    A = csr_of(S, random_dense(rng, n, p), p)
    c = S.charpoly(A)
    with S.DeviceCSR(A) as dA, S.DeviceCSR(csr_of(S, np.eye(n, dtype=np.int64), p)) as one:
        R = one.lincomb(1)
        for k in range(n - 1, -1, -1):   # Horner
            R = (R @ dA).lincomb(1, int(c[k]), one)
        assert R.shape == (n, n) and R.nnz == 0


# ---------------------------------------------------------------------------------------------
# batches, routes, repeats, counters
# ---------------------------------------------------------------------------------------------
def test_batch_mixing_all_classes_and_primes(S):
    rng = np.random.default_rng(0xCB00)
    cases = [(0, 127), (1, P32), (5, 3), (31, P16), (32, P32), (40, 5), (63, P31), (64, 127), (90, P32), (110, P16), (111, P31), (140, 3), (181, P32)]
    dense = [random_dense(rng, n, p) if n < 100 else random_sparse(rng, n, p, 6) for n, p in cases]
    mats = [csr_of(S, D, p) for D, (n, p) in zip(dense, cases)]
    out = S.charpoly_batch(mats)
    st = S.charpoly_stats()
    assert st["items"] == len(cases) and st["lds_path"] == len(cases) and st["global_path"] == 0 and st["launches"] == 4
    assert st["global_device_us"] == 0 and st["spare0"] == 0 and st["spare1"] == 0
    for got, D, (n, p) in zip(out, dense, cases):
        check(got, host_charpoly(D, p), p)


def test_batch_mixing_both_paths_routes_repeats_and_counters(S):
    rng = np.random.default_rng(0xCB01)
    cases = [(181, P16), (182, P32), (200, P16), (30, 127)]
    dense = [random_dense(rng, n, p) for n, p in cases]
    mats = [csr_of(S, D, p) for D, (n, p) in zip(dense, cases)]
    out = S.charpoly_batch(mats)
    st = S.charpoly_stats()
    assert (st["items"], st["lds_path"], st["global_path"], st["launches"]) == (4, 2, 2, 3)
    for got, D, (n, p) in zip(out, dense, cases):
        check(got, host_charpoly(D, p), p)
    # byte-identical repeats, and the three routes
    again = S.charpoly_batch(mats)
    for a, b, A in zip(out, again, mats):
        assert a.tobytes() == b.tobytes()
        assert S.charpoly(A).tobytes() == a.tobytes()
        with S.DeviceCSR(A) as dA:
            assert dA.charpoly().tobytes() == a.tobytes()
            assert S.charpoly(dA).tobytes() == a.tobytes()
    st = S.charpoly_stats()   # of the last call: one resident 30 x 30 matrix
    assert (st["items"], st["lds_path"], st["global_path"], st["launches"]) == (1, 1, 0, 1)
    S.charpoly(mats[1])
    st = S.charpoly_stats()
    assert (st["items"], st["lds_path"], st["global_path"], st["launches"]) == (1, 0, 1, 1) and st["lds_device_us"] == 0


def test_a_matrix_over_the_limit_is_refused_and_no_slot_is_written(S):
    p = P16
    small = csr_of(S, [[1, 2], [3, 4]], p)
    big = S.CSR.from_rows([[(0, 1)]] + [[] for _ in range(1024)], 1025, prime=p)
    with pytest.raises(S.SpasmError, match=r"matrix 1: characteristic polynomial limited to n <= 1024 \(n = 1025\)"):
        S.charpoly_batch([small, big, small])
    bufs = [(C.c_int32 * 4)(*([SENTINEL] * 4)) for _ in range(3)]
    ptrs = (C.POINTER(C.c_int32) * 3)(*[C.cast(b, C.POINTER(C.c_int32)) for b in bufs])
    arr = (C.POINTER(S._abi.CsrStruct) * 3)(small.data, big.data, small.data)
    assert S._abi.lib().spasm_amd_charpoly_batch(3, arr, ptrs) == -1
    assert "matrix 1: characteristic polynomial limited to n <= 1024 (n = 1025)" in S._abi.last_error()
    assert all(b[i] == SENTINEL for b in bufs for i in range(4))
    with S.DeviceCSR(big) as dB:
        with pytest.raises(S.SpasmError, match=r"limited to n <= 1024 \(n = 1025\)"):
            dB.charpoly()
    # the largest size the entry accepts: the shift of 1024 rows
    n = 1024
    A = S.CSR.from_rows([[(i + 1, 1)] if i + 1 < n else [] for i in range(n)], n, prime=p)
    check(S.charpoly(A), [0] * n + [1], p)
