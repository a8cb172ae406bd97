"""GPU tests of rank and determinant by preconditioned Wiedemann (spasm_amd_precond_sequence / _wiedemann_rank* / _wiedemann_det*;
csrc/precond.hpp).  The sequences must give the bytes of tests/precond_ref.py; rank and determinant must give what the reference
gives for the same seed, and what Gaussian elimination in Python integers gives wherever the contract promises it.  Every input
and seed is chosen on the CPU first (module fixtures): a seed is kept when the reference alone reaches the true value with it.

Two things the shapes of the issue do not allow, and what stands in their place:
  * mode 0 (D A) needs a square matrix, so the byte test runs it on a 70 x 70 matrix built like the 70 x 45 and the 45 x 70 one;
  * there is no odd permutation of one point: the permutation case starts at n = 2.
The identity is separated because the words of a diagonal differ from each other while n < p (the generator is a permutation
of 1 .. p - 1); where they cannot, the identity of order 130 over GF(127), device and reference must both stay at status 0."""
import numpy as np
import pytest

import precond_ref as R
import sparse_worst_cases as SW
from wiedemann_ref import Mat, bal

pytestmark = pytest.mark.gpu

P7, P16, P31, P32 = 127, 65521, 2**31 - 1, 4294967291
SEQ_PRIMES = (P7, P16, P31, P32)
SEQ_K = (1, 3, 8, 64)
SPMV_SEG = 16384


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def classes_matrix(n, m, p, rng):
    """n x m, n, m >= 39: row lengths AND column lengths include 0, 1, 32 and 33 (short and medium rows in both views); the
    entries are any int32 that is not a multiple of p (a multiple is dropped on upload and would shorten its row)"""
    mask = np.zeros((n, m), dtype=bool)
    mask[4:, 4:] = rng.random((n - 4, m - 4)) < 0.08
    mask[5, 1] = mask[1, 5] = True           # column 1 and row 1: one entry
    mask[6:38, 2] = mask[2, 6:38] = True     # column 2 and row 2: 32
    mask[6:39, 3] = mask[3, 6:39] = True     # column 3 and row 3: 33
    for lens in (mask.sum(axis=1), mask.sum(axis=0)):
        assert {0, 1, 32, 33} <= set(lens.tolist())
    vals = SW.rand_int32(rng, (n, m)).astype(np.int64)
    vals[vals % p == 0] = 1
    return Mat.from_dense(np.where(mask, vals, 0))


def arrow(p, rng):
    """n = m = 16500: row 0 and column 0 full (longer than SPMV_SEG: long rows in both views), the diagonal non-zero on the
    indices 0 .. 19.  Rank 21 for any non-zero values: the rows >= 20 span e_0, rows 1 .. 19 then give e_1 .. e_19, and row 0
    minus those keeps its non-zero entries in the columns >= 20."""
    n = 16500
    assert n > SPMV_SEG
    rows = [[(j, int(rng.integers(1, p))) for j in range(n)]]
    for i in range(1, n):
        r = [(0, int(rng.integers(1, p)))]
        if i < 20:
            r.append((i, int(rng.integers(1, p))))
        rows.append(r)
    return Mat.from_rows(rows, n), 21


def sqrt_of_minus_sum(p, rng):
    """a column y with y . y = 0 mod p, no zero entry"""
    if p % 4 == 1:
        while True:
            g = int(rng.integers(2, p))
            if pow(g, (p - 1) // 2, p) == p - 1:
                return [1, pow(g, (p - 1) // 4, p)]
    while True:
        a, b = int(rng.integers(1, p)), int(rng.integers(1, p))
        t = (-(a * a + b * b)) % p
        if t and pow(t, (p - 1) // 2, p) == 1:
            return [a, b, pow(t, (p + 1) // 4, p)]


def planted(n, m, r, p, rng):
    if r == 0:
        return np.zeros((n, m), dtype=np.int64)
    L = rng.integers(0, p, size=(n, r)).astype(object)
    Rt = rng.integers(0, p, size=(r, m)).astype(object)
    return np.array(((L @ Rt) % p).tolist(), dtype=np.int64)


RANK_SHAPES = [(7, 9, 0), (20, 30, 1), (25, 40, 25), (40, 25, 25), (None, None, None), (60, 90, 37), (33, 33, 33), (33, 33, 20),
               (1, 1, 1), (50, 20, 5), (17, 64, 16), (45, 45, 44)]


def rank_inputs(p):
    """12 (dense matrix, true rank, seed): the seed is the first with which the reference reaches the rank on its first try"""
    rng = np.random.default_rng(31337 + p % 1009)
    out = []
    for n, m, r in RANK_SHAPES:
        if n is None:   # the isotropic case: A = y z^T with y . y = 0, so A^T A = 0 and E A^T A is the zero matrix
            y = sqrt_of_minus_sum(p, rng)
            y = y + [0] * (12 - len(y))
            z = [int(x) for x in rng.integers(1, p, size=8)]
            D = np.array([[a * b % p for b in z] for a in y], dtype=np.int64)
            AtA = (D.astype(object).T @ D.astype(object)) % p
            assert not AtA.any() and D.any()
        else:
            D = planted(n, m, r, p, rng)
        true = R.eliminate(D, p)[0]
        M = Mat.from_dense(D)
        for seed in range(8):
            if R.rank(M, p, seed=seed, tries=1)[0] == true:
                break
        else:
            raise AssertionError("no seed below 8 reaches the rank on the host")
        out.append((D, true, seed))
    ranks = [t for _, t, _ in out]
    assert 0 in ranks and 1 in ranks and any(t == min(D.shape) and t > 1 for D, t, _ in out)
    return out


def small_prime_inputs(p):
    """20 (dense, true rank), and for p = 3 a 21st where seed 0 falls short and the maximum over three tries does not (None when
    the search finds none)"""
    rng = np.random.default_rng(77 + p)
    out = []
    for i in range(20):
        n, m = int(rng.integers(1, 21)), int(rng.integers(1, 31))
        D = planted(n, m, int(rng.integers(0, min(n, m) + 1)), p, rng)
        out.append((D, R.eliminate(D, p)[0]))
    extra = None
    for _ in range(60):
        n, m = int(rng.integers(3, 13)), int(rng.integers(3, 13))
        D = planted(n, m, int(rng.integers(1, min(n, m) + 1)), p, rng)
        true, M = R.eliminate(D, p)[0], Mat.from_dense(D)
        if R.rank(M, p, seed=0, tries=1)[0] < true and R.rank(M, p, seed=0, tries=3)[0] == true:
            extra = (D, true)
            break
    return out, extra


DET_N = (1, 2, 33, 64)


def odd_permutation(n):
    """n even: one n-cycle; n odd: an (n - 1)-cycle and a fixed point.  Both have parity -1."""
    c = n if n % 2 == 0 else n - 1
    D = np.zeros((n, n), dtype=np.int64)
    for i in range(c):
        D[i, (i + 1) % c] = 1
    if c < n:
        D[n - 1, n - 1] = 1
    return D


def det_inputs(p, n):
    """kind -> (dense, true determinant in [0, p), seed or None): the seed is the first below 6 with which the reference ends at
    status 1 within three tries"""
    rng = np.random.default_rng(555 + p % 1013 + n)
    cases = {}
    while True:
        Q = rng.integers(0, p, size=(n, n))
        if R.eliminate(Q, p)[1] != 0:
            break
    cases["non-singular"] = Q
    cases["identity"] = np.eye(n, dtype=np.int64)
    if n >= 2:
        cases["odd permutation"] = odd_permutation(n)
        Sg = Q.copy()
        Sg[n - 1] = [3 * int(a) % p for a in Q[0]]   # the last row is three times the first
        cases["singular"] = Sg
    else:
        cases["singular"] = np.zeros((1, 1), dtype=np.int64)
    out = {}
    for kind, D in cases.items():
        true = R.eliminate(D, p)[1]
        M, found = Mat.from_dense(D), None
        for seed in range(6):
            if R.det(M, p, seed=seed, tries=3)[1] == 1:
                found = seed
                break
        out[kind] = (D, true, found)
    assert out["identity"][1] == 1 and out["singular"][1] == 0
    assert n < 2 or out["odd permutation"][1] == p - 1
    return out


@pytest.fixture(scope="module")
def rank_cases():
    return {p: rank_inputs(p) for p in (P16, P32)}


@pytest.fixture(scope="module")
def det_cases():
    return {(p, n): det_inputs(p, n) for p in SEQ_PRIMES for n in DET_N}


@pytest.fixture(scope="module")
def arrows():
    """p -> (Mat, rank, seed): the first seed with which the reference, held to maxdeg = 24, returns the rank on its first try"""
    out = {}
    for p in (P16, P32):
        M, true = arrow(p, np.random.default_rng(p % 1000))
        for seed in range(8):
            if R.rank(M, p, seed=seed, tries=1, maxdeg=24)[0] == true:
                break
        else:
            raise AssertionError("no seed below 8 reaches the rank of the arrow on the host")
        out[p] = (M, true, seed)
    return out


# ---------------------------------------------------------------------------------------------
# sequences, byte for byte
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", SEQ_PRIMES)
def test_sequences_match_the_reference_byte_for_byte(S, p):
    rng = np.random.default_rng(1000 + p % 997)
    length = 5
    for n, m in ((70, 45), (45, 70), (70, 70)):
        M = classes_matrix(n, m, p, rng)
        with S.SpMV(M.csr(S, p, reduce=False)) as op:
            for K in SEQ_K:
                U, V = SW.rand_int32(rng, (m, K)), SW.rand_int32(rng, (m, K))
                dl, dr = SW.rand_int32(rng, (n, 1)).reshape(-1), SW.rand_int32(rng, (m, 1)).reshape(-1)
                modes = (0, 1) if n == m else (1,)
                for mode in modes:
                    want = R.sequence(M, mode, dl, dr, U, V, length, p)
                    got = op.precond_sequence(mode, dl, dr if mode else None, U, V, length)
                    assert got.dtype == np.int32 and got.shape == (length, K)
                    assert got.tobytes() == want.tobytes(), (n, m, K, mode)
                    assert op.precond_sequence(mode, dl, dr, U, V, length).tobytes() == got.tobytes(), (n, m, K, mode)   # twice
                    st = S.precond_stats()
                    assert (st["n"], st["m"], st["K"], st["products"]) == (n, m, K, (length - 1) * (1 + mode))
                    assert st["launches"] >= 2 * st["products"]   # a short and a medium class in either view
    with S.SpMV(classes_matrix(70, 45, p, rng).csr(S, p, reduce=False)) as op:
        with pytest.raises(S.SpasmError, match=r"not square \(70 x 45\)"):
            op.precond_sequence(0, np.ones(70, np.int32), None, np.ones((45, 1), np.int32), np.ones((45, 1), np.int32), 3)


@pytest.mark.parametrize("p", (P16, P32))
def test_long_rows_in_both_views(S, arrows, p):
    M, true, seed = arrows[p]
    n, K, length = M.n, 3, 2 * 24 + 2
    rng = np.random.default_rng(5 + p % 991)
    U, V = SW.rand_int32(rng, (n, K)), SW.rand_int32(rng, (n, K))
    dl, dr = SW.rand_int32(rng, (n, 1)).reshape(-1), SW.rand_int32(rng, (n, 1)).reshape(-1)
    A = M.csr(S, p)
    with S.SpMV(A) as op:
        for mode in (1, 0):
            want = R.sequence(M, mode, dl, dr, U, V, length, p)
            got = op.precond_sequence(mode, dl, dr, U, V, length)
            assert got.tobytes() == want.tobytes(), mode
            st = S.precond_stats()
            assert st["products"] == (length - 1) * (1 + mode) and st["launches"] >= 3 * st["products"]   # short, segments, combine
        want = R.rank(M, p, seed=seed, tries=1, maxdeg=24)
        assert want[0] == true == 21 and not want[1]
        assert op.wiedemann_rank(seed=seed, tries=1, maxdeg=24) == (true, False)
    assert S.wiedemann_rank(A, seed=seed, tries=1, maxdeg=24) == (true, False)


# ---------------------------------------------------------------------------------------------
# rank
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", (P16, P32))
def test_rank_equals_the_reference_and_the_true_rank(S, rank_cases, p):
    for i, (D, true, seed) in enumerate(rank_cases[p]):
        M = Mat.from_dense(D)
        n, m = D.shape
        want, certain, used = R.rank(M, p, seed=seed, tries=1)
        assert want == true, i
        A = M.csr(S, p)
        got = S.wiedemann_rank(A, seed=seed, tries=1)
        assert got == (true, certain) and got[1] == (true == min(n, m)), (i, got)
        st = S.precond_stats()
        md = min(n, m)
        assert (st["n"], st["m"], st["K"], st["tries"]) == (n, m, 8, 1), i
        assert st["products"] == 2 * (2 * md + 1) and st["launches"] >= st["products"], (i, st)
        assert st["degree"] - st["x_multiplicity"] == true, (i, st)
        with S.SpMV(A) as op:
            assert op.wiedemann_rank(seed=seed, tries=1) == got, i
        with S.DeviceCSR(A) as Dv:
            assert Dv.wiedemann_rank(seed=seed, tries=1) == got, i
        assert S.wiedemann_rank(A, seed=seed) == got, i   # more tries never lower the bound, and cannot raise it past the rank
        for md in (true - 1, true - 2):   # true - 1 is the edge the two extra terms are there for
            if md < 1:
                continue
            with pytest.raises(R.Refused):
                R.rank(M, p, seed=seed, tries=1, maxdeg=md)
            with pytest.raises(S.SpasmError, match="degree bound too small"):
                S.wiedemann_rank(A, seed=seed, tries=1, maxdeg=md)


@pytest.mark.parametrize("p", (3, P7))
def test_small_primes_keep_the_contract(S, p):
    """result <= rank and result == reference for 20 matrices; equality with the rank is not asserted.  The 21st input of p = 3
    is one where seed 0 alone falls short and the maximum over three tries reaches the rank (the search of small_prime_inputs
    finds one for either prime)."""
    cases, extra = small_prime_inputs(p)
    for i, (D, true) in enumerate(cases):
        M = Mat.from_dense(D)
        want, certain, _ = R.rank(M, p, seed=0, tries=3)
        got = S.wiedemann_rank(M.csr(S, p), seed=0, tries=3)
        assert got[0] <= true, (i, got, true)
        assert got == (want, certain), (i, got, want)
    assert extra is not None
    if extra is not None:
        D, true = extra
        A = Mat.from_dense(D).csr(S, p)
        one = S.wiedemann_rank(A, seed=0, tries=1)
        assert one[0] < true and one[0] == R.rank(Mat.from_dense(D), p, seed=0, tries=1)[0]
        assert S.wiedemann_rank(A, seed=0, tries=3)[0] == true


# ---------------------------------------------------------------------------------------------
# determinant
# ---------------------------------------------------------------------------------------------
def check_det(S, D, true, seed, p):
    M = Mat.from_dense(D)
    n = M.n
    A = M.csr(S, p)
    want = R.det(M, p, seed=seed, tries=3)
    got = S.wiedemann_det(A, seed=seed, tries=3)
    assert got == want[:2]
    assert got[1] == 1
    assert got[0] % p == true
    assert S.det(A) % p == true
    st = S.precond_stats()
    assert (st["n"], st["K"], st["tries"], st["products"]) == (n, 8, want[2], want[2] * (2 * n - 1))
    with S.SpMV(A) as op:
        assert op.wiedemann_det(seed=seed, tries=3) == got
    with S.DeviceCSR(A) as Dv:
        assert Dv.wiedemann_det(seed=seed, tries=3) == got


@pytest.mark.parametrize("n", DET_N)
@pytest.mark.parametrize("p", SEQ_PRIMES)
def test_determinant_of_regular_permutation_and_singular_matrices(S, det_cases, p, n):
    for kind in ("non-singular", "odd permutation", "singular"):
        if kind not in det_cases[(p, n)]:
            continue
        D, true, seed = det_cases[(p, n)][kind]
        assert seed is not None, kind
        check_det(S, D, true, seed, p)


@pytest.mark.parametrize("n", DET_N)
@pytest.mark.parametrize("p", SEQ_PRIMES)
def test_determinant_of_the_identity(S, det_cases, p, n):
    """The minimal polynomial of I is x - 1 and its characteristic polynomial (x - 1)^n: D separates them because its n < p words
    differ from each other."""
    D, true, seed = det_cases[(p, n)]["identity"]
    assert len(set(R.diagonal(n, 0, 0, p))) == n
    assert seed is not None, "the reference does not reach status 1 with a seed below 6"
    check_det(S, D, true, seed, p)


def test_status_0_of_the_reference_is_status_0_on_the_device(S):
    """the identity of order 130 over GF(127) with one try: 130 words out of 126 repeat whatever the seed, so the degree stays
    below n and x does not divide f"""
    p, n = P7, 130
    M = Mat.from_dense(np.eye(n, dtype=np.int64))
    assert len(set(R.diagonal(n, 0, 0, p))) == p - 1 < n
    assert R.det(M, p, seed=0, tries=1)[:2] == (0, 0)
    assert S.wiedemann_det(M.csr(S, p), seed=0, tries=1) == (0, 0)
    st = S.precond_stats()
    assert st["tries"] == 1 and 0 < st["degree"] <= p - 1 and st["x_multiplicity"] == 0
