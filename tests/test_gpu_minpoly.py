"""GPU tests of the minimal polynomial by Wiedemann's method (spasm_amd_minpoly / _spmv_minpoly / _dcsr_minpoly; csrc/krylov.hpp).
The polynomial of every matrix is known by construction.  With explicit U and V the device must give the bytes of the host
Wiedemann of tests/wiedemann_ref.py; with the seeded vectors and p >= 65521 it must give the known polynomial (the host reference,
run on the same vectors, is asserted to give it too: the inputs and seeds below were kept because it does); for small primes only
what the contract promises is asserted: the result is monic, divides the known polynomial, and annihilates V."""
import numpy as np
import pytest

import wiedemann_ref as W
from wiedemann_ref import PRIMES, bal

pytestmark = pytest.mark.gpu

P16, P31, P32 = 65521, 2**31 - 1, 4294967291
BIG = (P16, P31, P32)
SMALLP = (3, 5, 127)


def hidden_companions(p):
    """C(f1) + C(f2) + C(f1) under a simultaneous permutation of rows and columns: minimal polynomial lcm(f1, f2), degree < n"""
    rng = np.random.default_rng(4242 + p % 1009)
    while True:
        f1, f2 = W.rand_monic(rng, 7, p), W.rand_monic(rng, 12, p)
        if f1[0] and f2[0] and W.pgcd(f1, f2, p) == [1]:
            break
    D = W.block_diag([W.companion(f1, p), W.companion(f2, p), W.companion(f1, p)])
    perm = rng.permutation(len(D))
    return D[np.ix_(perm, perm)], W.pmul(f1, f2, p)


def known_cases(p):
    """name -> (dense matrix, its minimal polynomial as residues in [0, p), low degree first)"""
    rng = np.random.default_rng(99 + p % 1013)
    cases = {}
    cases["identity"] = (np.eye(40, dtype=np.int64), [p - 1, 1])
    cases["zero"] = (np.zeros((30, 30), dtype=np.int64), [0, 1])
    cases["shift"] = (np.eye(50, k=1, dtype=np.int64), [0] * 50 + [1])
    cyc = np.zeros((3, 3), dtype=np.int64)
    cyc[0, 1] = cyc[1, 2] = cyc[2, 0] = 1
    cases["3-cycle"] = (cyc, [p - 1, 0, 0, 1])
    vals = [int(v) for v in rng.choice(min(p, 1000), size=min(5, p), replace=False)]
    diag = np.diag(np.array([vals[i % len(vals)] for i in range(300)], dtype=np.int64))
    mp = [1]
    for v in vals:
        mp = W.pmul(mp, [(-v) % p, 1], p)
    cases["diagonal"] = (diag, mp)
    cases["hidden companions"] = hidden_companions(p)
    f = W.rand_monic(rng, 200, p)
    cases["companion 200"] = (W.companion(f, p), f)
    return cases


def divides(g, f, p):
    return W.pdivmod([int(x) % p for x in f], [int(x) % p for x in g], p)[1] == []


@pytest.fixture(scope="module")
def cases():
    return {p: known_cases(p) for p in set(BIG + SMALLP + PRIMES)}


@pytest.mark.parametrize("p", BIG)
def test_default_seed_gives_the_known_polynomial(S, cases, p):
    for name, (D, mp) in cases[p].items():
        M = W.Mat.from_dense(D)
        U, V = S.minpoly_vectors(M.n, 8, 0, p)
        assert W.ref_minpoly(M, U, V, p) == mp, name   # the reference itself finds it with these vectors
        A = M.csr(S, p)
        got = S.minpoly(A)
        assert got.dtype == np.int32 and got.tolist() == bal(mp, p).tolist(), name
        assert S.minpoly(A).tobytes() == got.tobytes(), name   # the same seed twice
        st = S.minpoly_stats()
        assert (st["n"], st["K"], st["steps"], st["degree"], st["bm_class"]) == (M.n, 8, 2 * M.n - 1, len(mp) - 1, 1), name


@pytest.mark.parametrize("p", BIG)
def test_the_three_entries_agree_and_degree_n_is_the_charpoly(S, cases, p):
    D, mp = cases[p]["companion 200"]
    A = W.Mat.from_dense(D).csr(S, p)
    want = bal(mp, p).tolist()
    with S.SpMV(A) as op:
        assert op.minpoly().tolist() == want
    with S.DeviceCSR(A) as R:
        assert R.minpoly().tolist() == want
    assert S.charpoly(A).tolist() == want   # the degree is n: the minimal polynomial is the characteristic polynomial
    D, mp = cases[p]["hidden companions"]
    with S.DeviceCSR(W.Mat.from_dense(D).csr(S, p)) as R:
        assert R.minpoly(K=4, seed=1).tolist() == bal(mp, p).tolist()


@pytest.mark.parametrize("p", PRIMES)
def test_explicit_vectors_give_the_bytes_of_the_host_wiedemann(S, cases, p):
    rng = np.random.default_rng(7 + p % 1019)
    for name in ("shift", "3-cycle", "diagonal", "hidden companions"):
        D, mp = cases[p][name]
        M = W.Mat.from_dense(D)
        for K in (1, 3):
            U = bal(rng.integers(0, p, size=(M.n, K), dtype=np.int64), p)
            V = bal(rng.integers(0, p, size=(M.n, K), dtype=np.int64), p)
            want = W.ref_minpoly(M, U, V, p)
            got = S.minpoly(M.csr(S, p), K=K, U=U, V=V)
            assert got.tolist() == bal(want, p).tolist(), (name, K)
            assert divides(want, mp, p), (name, K)


# m(A) V = 0 is more than the contract promises: the projection by u may lose a factor of the minimal polynomial of v, and over
# GF(3) it does for one input with seed 0 (the host reference on the same vectors returns degree 199 of 200 there and does not
# annihilate V either).  The seeds are those for which the host reference annihilates V: 0, but for this input.
SMALL_SEEDS = {(3, "companion 200"): 1}


@pytest.mark.parametrize("p", SMALLP)
def test_small_primes_keep_the_contract(S, cases, p):
    for name, (D, mp) in cases[p].items():
        M = W.Mat.from_dense(D)
        A = M.csr(S, p)
        seed = SMALL_SEEDS.get((p, name), 0)
        got = S.minpoly(A, K=8, seed=seed)
        assert got[-1] == 1, name
        assert divides(got, mp, p), name
        U, V = S.minpoly_vectors(M.n, 8, seed, p)
        with S.SpMV(A) as op:
            assert not W.poly_apply(op, got, V, p).any(), name   # m(A) V = 0


def test_refusals_and_the_empty_matrix(S, cases):
    p = P16
    D, mp = cases[p]["hidden companions"]
    A = W.Mat.from_dense(D).csr(S, p)
    d = len(mp) - 1
    assert S.minpoly(A, maxdeg=d).tolist() == bal(mp, p).tolist()          # the exact bound is enough
    assert S.minpoly(A, maxdeg=d + 3).tolist() == bal(mp, p).tolist()
    with pytest.raises(S.SpasmError, match="spasm_amd_minpoly: degree bound too small"):
        S.minpoly(A, maxdeg=d - 1)
    with S.SpMV(A) as op:
        with pytest.raises(S.SpasmError, match="spasm_amd_spmv_minpoly: degree bound too small"):
            op.minpoly(maxdeg=d - 1)
    T = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)], []], 2, prime=127)
    with pytest.raises(S.SpasmError, match=r"spasm_amd_minpoly: not square \(3 x 2\)"):
        S.minpoly(T)
    with S.SpMV(T) as op:
        with pytest.raises(S.SpasmError, match=r"spasm_amd_spmv_minpoly: not square \(3 x 2\)"):
            op.minpoly()
    with S.DeviceCSR(T) as R:
        with pytest.raises(S.SpasmError, match=r"spasm_amd_dcsr_minpoly: not square \(3 x 2\)"):
            R.minpoly()
    E = S.CSR.from_rows([], 0, prime=p)
    assert S.minpoly(E).tolist() == [1]
    with S.SpMV(E) as op:
        assert op.minpoly().tolist() == [1]


def test_singularity_is_read_off_the_constant_term(S):
    """x divides the result exactly when it says the matrix is singular: a nilpotent block beside an invertible one"""
    p = P31
    rng = np.random.default_rng(1)
    f = W.rand_monic(rng, 20, p)
    f[0] = f[0] or 1
    D = W.block_diag([W.companion(f, p), np.eye(4, k=1, dtype=np.int64)])
    got = S.minpoly(W.Mat.from_dense(D).csr(S, p))
    assert got.tolist() == bal(W.pmul(f, [0, 0, 0, 0, 1], p), p).tolist() and got[0] == 0
    got = S.minpoly(W.Mat.from_dense(W.companion(f, p)).csr(S, p))
    assert got.tolist() == bal(f, p).tolist() and got[0] != 0
