"""GPU tests of block Horner and the block Wiedemann solve (spasm_amd_block_poly_apply / _dev, _block_wiedemann_solve*,
_block_solve_stats; csrc/block_horner.hpp).  block_poly_apply is compared byte for byte with the restatement in Python integers
(tests/block_solve_ref.py); for the matrix with a long row, whose dense form no Python loop can walk, with exact numpy products.
The solve runs on the inputs of tests/block_solve_cases.py, which tests/test_block_solve_abi.py shows the reference to decide at
try 0 of the same seed: the device must give status 1 everywhere and the unique solution.  Larger systems are checked by the
residual in exact numpy products; over GF(3) only soundness is asserted."""
import ctypes as C

import numpy as np
import pytest

import block_solve_cases as K
import block_solve_ref as BS
import wiedemann_ref as W
from block_solve_cases import P3, P16, P32
from test_gpu_block_wiedemann import long_row_matrix, rand_bal, short_rows_matrix
from wiedemann_ref import bal

pytestmark = pytest.mark.gpu

PRIMES3 = (P3, P16, P32)


def np_block_poly_apply(M, Cs, V, p):
    """sum_t M^t V C[t] by block Horner in exact numpy int64 arithmetic -> balanced int32 (n, K)"""
    Vr = np.asarray(V, dtype=np.int64) % p
    Cr = np.asarray(Cs, dtype=np.int64) % p
    Y = None
    for Ct in Cr[::-1]:
        VC = np.zeros((M.n, Ct.shape[1]), dtype=np.int64)
        for c in range(Ct.shape[0]):   # 16 terms below 2^32 each
            VC += W.mulmod(np.broadcast_to(Vr[:, c:c + 1], VC.shape).copy(), np.broadcast_to(Ct[c][None, :], VC.shape).copy(), p)
        Y = VC % p if Y is None else (M.apply(Y, p) + VC) % p
    return bal(Y, p)


def py_block_poly_apply(M, Cs, V, p, trans=False):
    D = K.dense_of(M.transpose() if trans else M)
    X = BS.block_poly_apply(D, [[[int(x) % p for x in row] for row in Ct] for Ct in Cs], [[int(x) for x in row] for row in V], p)
    return bal(np.array(X, dtype=object).reshape(M.n, -1), p)


# ---------------------------------------------------------------- block_poly_apply
@pytest.mark.parametrize("trans", (False, True))
@pytest.mark.parametrize("b,k", ((2, 1), (2, 2), (16, 1), (16, 16), (4, 3)))
@pytest.mark.parametrize("p", PRIMES3)
def test_block_poly_apply_matches_the_python_integers_on_short_rows(S, p, b, k, trans):
    rng = np.random.default_rng(131 * b + 7 * k + p % 1009 + int(trans))
    n = 70
    M = short_rows_matrix(rng, n, p, empty=True)
    # unreduced int32 words in V and C, the extremes among them
    V = rng.integers(-2**31, 2**31, size=(n, b), dtype=np.int64).astype(np.int32)
    V[0, 0], V[1, 0] = 2**31 - 1, -2**31
    V0 = V.copy()
    with S.SpMV(M.csr(S, p)) as op:
        for D in (-1, 0, 1, 5):
            Cs = rng.integers(-2**31, 2**31, size=(D + 1, b, k), dtype=np.int64).astype(np.int32)
            if D >= 0:
                Cs[0, 0, 0] = -2**31
            got = S.block_poly_apply(op, Cs, V, trans=trans)
            assert got.shape == (n, k) and got.dtype == np.int32
            if D < 0:
                assert not got.any()
                continue
            want = py_block_poly_apply(M, Cs, V, p, trans)
            assert got.tobytes() == want.tobytes(), D
            assert op.block_poly_apply(Cs, V, trans=trans).tobytes() == got.tobytes()   # two runs, the same bytes
            st = S.block_solve_stats()
            assert (st["n"], st["b"], st["K"], st["products"], st["horner_products"]) == (n, b, k, D, D)
    assert V.tobytes() == V0.tobytes()


@pytest.mark.parametrize("b,k,p,trans", [(16, 16, P32, False), (2, 1, P16, True), (4, 3, P3, False), (16, 5, P16, True), (8, 8, P32, True)])
def test_block_poly_apply_with_a_long_row_takes_the_segments_and_the_combine(S, b, k, p, trans):
    rng = np.random.default_rng(11 * b + k + p % 1013)
    n, D = 16400, 2
    M = long_row_matrix(rng, n, p)
    V = rand_bal(rng, (n, b), p)
    Cs = rand_bal(rng, (D + 1, b, k), p)
    want = np_block_poly_apply(M.transpose() if trans else M, Cs, V, p)
    with S.SpMV(M.csr(S, p)) as op:
        got = S.block_poly_apply(op, Cs, V, trans=trans)
        again = S.block_poly_apply(op, Cs, V, trans=trans)
    assert got.tobytes() == want.tobytes()
    assert again.tobytes() == got.tobytes()


def test_the_numpy_block_horner_is_the_python_integers():
    p, n, b, k = P32, 70, 16, 5
    rng = np.random.default_rng(9)
    M = short_rows_matrix(rng, n, p)
    V, Cs = rand_bal(rng, (n, b), p), rand_bal(rng, (3, b, k), p)
    assert np_block_poly_apply(M, Cs, V, p).tobytes() == py_block_poly_apply(M, Cs, V, p).tobytes()


@pytest.mark.parametrize("signs", ("plus", "minus", "mixed"))
def test_block_poly_apply_at_the_accumulator_bound(S, signs):
    """every word of V and C is +-(p - 1) / 2 at p = 4294967291, b = 16: sixteen products of 2^61.99 each in one combination"""
    p, n, b, k, h = P32, 70, 16, 16, (P32 - 1) // 2
    rng = np.random.default_rng(77)
    M = short_rows_matrix(rng, n, p, empty=True)
    M.v[:] = h if signs != "minus" else -h   # the row sums are at their extremes too
    sv = {"plus": (1, 1), "minus": (-1, 1), "mixed": (1, -1)}[signs]
    V = np.full((n, b), sv[0] * h, dtype=np.int32)
    Cs = np.full((2, b, k), sv[1] * h, dtype=np.int32)
    if signs == "mixed":
        V[::2] *= -1
        Cs[:, ::2] *= -1
    with S.SpMV(M.csr(S, p)) as op:
        got = S.block_poly_apply(op, Cs, V)
    assert got.tobytes() == py_block_poly_apply(M, Cs, V, p).tobytes()


def test_block_poly_apply_on_device_tensors_and_its_refusals(S):
    import torch

    p, n, b, k, D = P16, 300, 4, 3, 3
    rng = np.random.default_rng(5)
    M = short_rows_matrix(rng, n, p)
    V, Cs = rand_bal(rng, (n, b), p), rand_bal(rng, (D + 1, b, k), p)
    want = np_block_poly_apply(M, Cs, V, p)
    with S.SpMV(M.csr(S, p)) as op:
        assert S.block_poly_apply(op, Cs, V).tobytes() == want.tobytes()
        tV = torch.from_numpy(V).cuda()
        got = S.block_poly_apply(op, Cs, tV)
        assert got.device.type == "cuda" and got.cpu().numpy().tobytes() == want.tobytes()
        wide = torch.zeros((n, b + 3), dtype=torch.int32, device="cuda")   # a leading dimension above b
        wide[:, :b] = tV
        assert S.block_poly_apply(op, Cs, wide[:, :b], trans=True).cpu().numpy().tobytes() == np_block_poly_apply(M.transpose(), Cs, V, p).tobytes()
        lib, err = S._abi.lib(), S._abi.last_error
        who = "spasm_amd_block_poly_apply"
        X = np.full((n, k), 0x5A5A5A5A, dtype=np.int32)
        call = lambda tr=0, bb=b, kk=k, dd=D, cp=Cs.ctypes.data, vp=V.ctypes.data, ldv=b, xp=X.ctypes.data, ldx=k: lib.spasm_amd_block_poly_apply(
            op._op, tr, bb, kk, dd, cp, vp, ldv, xp, ldx)
        for bad in (0, 3, 32):
            assert call(bb=bad) == -1 and err() == f"{who}: b must be 2, 4, 8 or 16"
        for bad in (0, b + 1):
            assert call(kk=bad, ldx=b + 1) == -1 and err() == f"{who}: K out of range (1 <= K <= b)"
        assert call(tr=2) == -1 and err() == f"{who}: trans must be 0 or 1"
        for bad in (-2, 1 << 24):
            assert call(dd=bad) == -1 and err() == f"{who}: D out of range (-1 <= D < 2^24)"
        assert call(ldv=k - 1) == -1 and err() == f"{who}: ldv < b"
        assert call(ldv=b - 1) == -1 and err() == f"{who}: ldv < b"
        assert call(ldx=k - 1) == -1 and err() == f"{who}: ldx < K"
        assert call(cp=None) == -1 and err() == f"{who}: NULL array"
        assert call(vp=None) == -1 and err() == f"{who}: NULL array"
        assert call(xp=None) == -1 and err() == f"{who}: NULL array"
        assert (X == 0x5A5A5A5A).all()
        both = np.full((n, b + k), 0x5A5A5A5A, dtype=np.int32)   # X begins on the last word of a row of V
        assert call(vp=both.ctypes.data, ldv=b + k, xp=both.ctypes.data + 4 * (b - 1), ldx=b + k) == -1 and err() == f"{who}: V must not overlap X"
    tall = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)], []], 2, prime=127)
    with S.SpMV(tall) as op:
        with pytest.raises(S.SpasmError, match=r"not square \(3 x 2\)"):
            S.block_poly_apply(op, np.zeros((1, 2, 1), dtype=np.int32), np.zeros((3, 2), dtype=np.int32))


# ---------------------------------------------------------------- block_wiedemann_solve
def unique_solution(M, B, p, trans):
    D = K.dense_of(M.transpose() if trans else M)
    cols = [BS.solve_dense(D, [int(x) for x in B[:, j]], p) for j in range(B.shape[1])]
    return bal(np.array(cols, dtype=object).T.reshape(M.n, -1), p)


@pytest.mark.parametrize("trans", (False, True))
@pytest.mark.parametrize("n,b,k", K.SHAPES)
@pytest.mark.parametrize("p", (P16, P32))
def test_solve_decides_every_column_at_try_0_and_finds_the_unique_solution(S, p, n, b, k, trans):
    M, B = K.system(n, k, p)
    A = M.csr(S, p)
    want = unique_solution(M, B, p, trans)
    X, status = S.block_wiedemann_solve(A, B, b=b, trans=trans, seed=K.SEED, tries=1)
    assert status.tolist() == [1] * k
    assert X.dtype == np.int32 and X.tobytes() == want.tobytes()
    st = S.block_solve_stats()
    D = st["max_degree"]
    assert (st["n"], st["b"], st["K"], st["len"], st["tries"]) == (n, b, k, K.terms(n, b), 1)
    assert st["sequence_products"] == st["len"] - 1 and st["horner_products"] == max(D - 1, 0) + 1
    assert st["products"] == st["sequence_products"] + st["horner_products"]
    assert (st["solved"], st["kernel_vectors"]) == (k, 0) and st["degree_sum"] <= n and D <= st["len"]
    # the three entries agree, and two runs give the same bytes
    with S.SpMV(A) as op:
        X2, s2 = op.block_wiedemann_solve(B, b=b, trans=trans, seed=K.SEED, tries=1)
    X3, s3 = S.DeviceCSR(A).block_wiedemann_solve(B, b=b, trans=trans, seed=K.SEED, tries=1)
    X4, s4 = S.block_wiedemann_solve(A, B, b=b, trans=trans, seed=K.SEED, tries=1)
    for Xo, so in ((X2, s2), (X3, s3), (X4, s4)):
        assert Xo.tobytes() == X.tobytes() and so.tolist() == status.tolist()


def test_solve_takes_one_right_hand_side_as_a_vector_and_a_wide_b(S):
    p, (n, b, k) = P32, K.SHAPES[3]
    M, B = K.system(n, k, p)
    wide = np.full((n, k + 3), 12345, dtype=np.int32)
    wide[:, :k] = B
    X, status = S.block_wiedemann_solve(M.csr(S, p), wide[:, :k], b=b, seed=K.SEED)
    assert status.tolist() == [1] * k and all(K.residual_is_zero(M, X, B, p))
    x, s1 = S.block_wiedemann_solve(M.csr(S, p), B[:, 0].copy(), b=b, seed=K.SEED)
    assert x.shape == (n,) and s1.tolist() in ([1], [0])
    if s1[0] == 1:
        assert x.tobytes() == X[:, 0].tobytes()   # the solution is unique


@pytest.mark.parametrize("n,b,k", K.MID)
def test_solve_n_130_is_decided_at_try_0_like_the_reference(S, n, b, k):
    p = P16
    M, B = K.system(n, k, p)
    X, status = S.block_wiedemann_solve(M.csr(S, p), B, b=b, seed=K.SEED, tries=1)
    assert status.tolist() == [1] * k
    assert all(K.residual_is_zero(M, X, B, p))


@pytest.mark.parametrize("b", (4, 16))
@pytest.mark.parametrize("p", (P16, P32))
def test_solve_n_300_proves_every_column_within_three_tries(S, p, b):
    n = 300
    M, B = K.system(n, b, p)
    X, status = S.block_wiedemann_solve(M.csr(S, p), B, b=b, seed=K.SEED, tries=3)
    assert (status != 0).all()
    ok = K.residual_is_zero(M, X, B, p)
    assert all(ok[j] for j in range(b) if status[j] == 1)
    st = S.block_solve_stats()
    assert st["products"] == st["sequence_products"] + st["horner_products"] and st["sequence_products"] == (st["len"] - 1) * st["tries"]
    assert st["solved"] == int((status == 1).sum()) and st["kernel_vectors"] == int((status == 2).sum())


@pytest.mark.parametrize("kind,b,k", K.SPECIAL)
@pytest.mark.parametrize("p", (P16, P32))
def test_solve_the_identity_and_a_permutation_by_the_residual(S, p, kind, b, k):
    M, B = K.special(kind, k, p)
    X, status = S.block_wiedemann_solve(M.csr(S, p), B, b=b, seed=K.SEED, tries=1)
    assert status.tolist() == [1] * k
    assert all(K.residual_is_zero(M, X, B, p))
    if kind == "identity":
        assert X.tobytes() == B.tobytes()


@pytest.mark.parametrize("p", (P16, P32))
def test_solve_the_planted_singular_matrix(S, p):
    n, b = K.SINGULAR
    M, B = K.system(n, 2, p, kind="singular")
    X, status = S.block_wiedemann_solve(M.csr(S, p), B, b=b, seed=K.SEED, tries=1)
    assert status.tolist() == [1, 2]
    assert K.residual_is_zero(M, X[:, :1], B[:, :1], p) == [True]
    assert X[:, 1].any() and K.residual_is_zero(M, X[:, 1:], None, p, regular=False) == [True]
    st = S.block_solve_stats()
    assert (st["solved"], st["kernel_vectors"]) == (1, 1)


@pytest.mark.parametrize("kind,n,b,k", [("random", 5, 2, 2), ("random", 30, 4, 4), ("random", 64, 8, 5), ("singular", 24, 2, 2),
                                        ("singular", 40, 16, 16), ("random", 1, 2, 1)])
def test_solve_over_gf3_is_sound_whatever_it_decides(S, kind, n, b, k):
    p = P3
    M, B = K.system(n, k, p, kind=kind if n > 2 else "random")
    X, status = S.block_wiedemann_solve(M.csr(S, p), B, b=b, seed=2, tries=3)
    solved = K.residual_is_zero(M, X, B, p)
    kernel = K.residual_is_zero(M, X, None, p, regular=False)
    for j in range(k):
        assert status[j] in (0, 1, 2)
        if status[j] == 1:
            assert solved[j]
        elif status[j] == 2:
            assert kernel[j] and X[:, j].any()
        else:
            assert not X[:, j].any()
    st = S.block_solve_stats()
    assert st["solved"] == int((status == 1).sum()) and st["kernel_vectors"] == int((status == 2).sum())
    assert 1 <= st["tries"] <= 3 and st["sequence_products"] == (st["len"] - 1) * st["tries"]
