"""CPU tests of the block solve boundary (spasm_amd_block_poly_apply* / _block_wiedemann_solve* / _block_solve_stats): symbols and
bindings, the argument checks that come before anything touches a device, the empty system that needs none, and the Python
restatement (tests/block_solve_ref.py) run on the inputs of tests/test_gpu_block_solve.py (tests/block_solve_cases.py) with the
seeded vectors of try 0: it decides every one of them, so the GPU test may ask the device for the same.  Nothing here needs a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import block_solve_cases as K
import block_solve_ref as BS
import block_wiedemann_ref as R

SENTINEL = 0x5A5A5A5A
SYMBOLS = [
    "spasm_amd_block_poly_apply", "spasm_amd_block_poly_apply_dev", "spasm_amd_block_wiedemann_solve",
    "spasm_amd_spmv_block_wiedemann_solve", "spasm_amd_dcsr_block_wiedemann_solve", "spasm_amd_block_solve_stats",
]


def test_block_solve_symbols_exported_with_the_documented_signatures(S):
    lib = S._abi.lib()
    for name in SYMBOLS:
        assert name in S._abi.SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.restype == S._abi.SIGNATURES[name][0] and fn.argtypes == S._abi.SIGNATURES[name][1], name
    for name in ("block_poly_apply", "block_wiedemann_solve", "block_solve_stats"):
        assert callable(getattr(S, name)), name
        assert name in S.__all__, name
    assert callable(S.SpMV.block_poly_apply) and callable(S.SpMV.block_wiedemann_solve) and callable(S.DeviceCSR.block_wiedemann_solve)
    assert len(S.api.BLOCK_SOLVE_STATS) == 16 and len(set(S.api.BLOCK_SOLVE_STATS)) == 16
    assert len(S.api.BLOCK_STATS) == 10   # the determinant's counter block keeps its slots
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spasm_amd.h")).read()
    for decl in (
        "int spasm_amd_block_poly_apply(spasm_amd_spmv *op, int trans, int b, int K, int D, const spasm_ZZp *coef, const spasm_ZZp *V, i64 ldv,",
        "int spasm_amd_block_poly_apply_dev(spasm_amd_spmv *op, int trans, int b, int K, int D, const spasm_ZZp *coef, const spasm_ZZp *V, i64 ldv,",
        "int spasm_amd_block_wiedemann_solve(const struct spasm_csr *A, int trans, int b, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries,",
        "int spasm_amd_spmv_block_wiedemann_solve(spasm_amd_spmv *op, int trans, int b, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries,",
        "int spasm_amd_dcsr_block_wiedemann_solve(const spasm_amd_dcsr *D, int trans, int b, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries,",
        "void spasm_amd_block_solve_stats(i64 *out);",
        "IS PROVED",
    ):
        assert decl in hdr, decl


def test_argument_checks_that_fail_before_any_device(S):
    lib = S._abi.lib()
    err = S._abi.last_error
    n = 2
    sq = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)]], 2, prime=127)
    tall = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)], []], 2, prime=127)
    B = (C.c_int32 * 64)(*([1] * 64))
    X = (C.c_int32 * 64)(*([SENTINEL] * 64))
    status = (C.c_int32 * 16)(*([-7] * 16))
    untouched = lambda: list(X) == [SENTINEL] * 64 and list(status) == [-7] * 16
    solve = lib.spasm_amd_block_wiedemann_solve
    who = "spasm_amd_block_wiedemann_solve"

    # NULL handles
    for name in ("spasm_amd_block_wiedemann_solve", "spasm_amd_dcsr_block_wiedemann_solve"):
        assert getattr(lib, name)(None, 0, 2, 1, B, 1, 0, 3, X, 1, status) == -1 and err() == f"{name}: NULL matrix"
    assert lib.spasm_amd_spmv_block_wiedemann_solve(None, 0, 2, 1, B, 1, 0, 3, X, 1, status) == -1
    assert err() == "spasm_amd_spmv_block_wiedemann_solve: NULL operator"
    assert lib.spasm_amd_block_poly_apply(None, 0, 2, 1, 0, B, B, 2, X, 1) == -1 and err() == "spasm_amd_block_poly_apply: NULL operator"
    assert lib.spasm_amd_block_poly_apply_dev(None, 0, 2, 1, 0, B, B, 2, X, 1, None) == -1
    assert err() == "spasm_amd_block_poly_apply_dev: NULL operator"
    # the block widths
    for b in (0, 1, 3, 5, 12, 32, -2):
        assert solve(sq.data, 0, b, 1, B, 1, 0, 3, X, 1, status) == -1 and err() == f"{who}: b must be 2, 4, 8 or 16"
    # K outside 1 .. b
    for b, k in ((2, 0), (2, -1), (2, 3), (4, 5), (16, 17)):
        assert solve(sq.data, 0, b, k, B, 32, 0, 3, X, 32, status) == -1 and err() == f"{who}: K out of range (1 <= K <= b)"
    # trans
    for tr in (-1, 2):
        assert solve(sq.data, tr, 2, 2, B, 2, 0, 3, X, 2, status) == -1 and err() == f"{who}: trans must be 0 or 1"
    # leading dimensions
    assert solve(sq.data, 0, 2, 2, B, 1, 0, 3, X, 2, status) == -1 and err() == f"{who}: ldb < K"
    assert solve(sq.data, 0, 2, 2, B, 2, 0, 3, X, 1, status) == -1 and err() == f"{who}: ldx < K"
    # NULL arrays
    assert solve(sq.data, 0, 2, 2, None, 2, 0, 3, X, 2, status) == -1 and err() == f"{who}: NULL array"
    assert solve(sq.data, 0, 2, 2, B, 2, 0, 3, None, 2, status) == -1 and err() == f"{who}: NULL array"
    assert solve(sq.data, 0, 2, 2, B, 2, 0, 3, X, 2, None) == -1 and err() == f"{who}: NULL array"
    # a square matrix
    assert solve(tall.data, 0, 2, 2, B, 2, 0, 3, X, 2, status) == -1 and err() == f"{who}: not square (3 x 2)"
    assert untouched()
    with pytest.raises(S.SpasmError, match=r"not square \(3 x 2\)"):
        S.block_wiedemann_solve(tall, np.zeros((3, 2), dtype=np.int32), b=2)
    with pytest.raises(S.SpasmError, match="b must be 2, 4, 8 or 16"):
        S.block_wiedemann_solve(sq, np.zeros((n, 2), dtype=np.int32), b=3)
    with pytest.raises(S.SpasmError, match=r"K out of range \(1 <= K <= b\)"):
        S.block_wiedemann_solve(sq, np.zeros((n, 3), dtype=np.int32), b=2)
    # the wrappers' own checks
    with pytest.raises(TypeError):
        S.block_wiedemann_solve(np.zeros((2, 2)), np.zeros((2, 1), dtype=np.int32))
    with pytest.raises(TypeError):
        S.block_wiedemann_solve(sq, np.zeros((2, 1)))
    with pytest.raises(TypeError):
        S.block_poly_apply(None, np.zeros((1, 2, 1), dtype=np.int32), np.zeros((2, 2), dtype=np.int32))
    assert S.block_solve_stats() == {k: 0 for k in S.api.BLOCK_SOLVE_STATS}


def test_block_poly_apply_checks_need_an_operator_and_are_made_of_the_same_words(S):
    """block_poly_apply takes a resident operator, which needs a device: its refusals beyond the NULL operator (b, K, trans, D, ldv,
    ldx, NULL arrays, not square, overlap) are run in tests/test_gpu_block_solve.py.  Here: the header documents every one."""
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spasm_amd.h")).read()
    start = hdr.index("---- block Horner and the block Wiedemann solve")
    doc = " ".join(hdr[start:].split())
    for words in ('"b must be 2, 4, 8 or 16"', '"K out of range (1 <= K <= b)"', '"trans must be 0 or 1"', "(-1 <= D < 2^24)", '"ldv < b"',
                  '"ldb < K"', '"ldx < K"', '"V must not overlap X"', "not square (3 x 2)"):
        assert words in doc, words


def test_the_empty_system_is_solved_without_a_device(S):
    E = S.CSR.from_rows([], 0, prime=65521)
    X, status = S.block_wiedemann_solve(E, np.zeros((0, 3), dtype=np.int32), b=4)
    assert X.shape == (0, 3) and status.tolist() == [1, 1, 1]
    assert S._abi.last_error() == ""
    st = S.block_solve_stats()
    assert (st["b"], st["K"], st["solved"], st["products"], st["tries"]) == (4, 3, 3, 0, 0)


def test_block_solve_fails_loudly_without_gpu(S):
    if S._abi.lib().spasm_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    sq = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)]], 2, prime=127)
    B = np.ones((2, 1), dtype=np.int32)
    X = np.full((2, 1), SENTINEL, dtype=np.int32)
    status = np.full(1, -7, dtype=np.int32)
    assert S._abi.lib().spasm_amd_block_wiedemann_solve(sq.data, 0, 2, 1, B.ctypes.data, 1, 0, 3, X.ctypes.data, 1, status.ctypes.data) == -1
    assert S._abi.last_error().startswith("spasm_amd_block_wiedemann_solve") and "no HIP device" in S._abi.last_error()
    assert (X == SENTINEL).all() and status[0] == -7
    with pytest.raises(S.SpasmError, match="no HIP device"):
        S.block_wiedemann_solve(sq, B, b=2)


# ---------------------------------------------------------------- the reference on itself
def test_the_reduction_of_g_finds_regular_columns_and_null_vectors():
    p = 101
    # rank 2: rows 0 and 1 independent, row 2 = row 0 + row 1; e_0 lies in the row space, e_1 and e_2 do not
    G = [[1, 0, 0], [0, 1, 1], [1, 1, 1]]
    g, t, rank, pivrow = BS.reduce_g(G, p)
    assert rank == 2 and pivrow == [0, 1, -1]
    assert R.mat_mul(t, G, p) == g and g[2] == [0, 0, 0]
    combos = BS.combinations([G], p, 3)
    assert [c[0] for c in combos] == [True, False, False]
    assert combos[0][1][0] == [1, 0, 0] and combos[1][1][0] == [0, 0, 0]
    # a non-singular G: every column is regular and lambda_j is row j of the inverse
    G = [[2, 1], [1, 1]]
    assert [c[0] for c in BS.combinations([G], p, 2)] == [True, True]
    _, t, rank, _ = BS.reduce_g(G, p)
    assert rank == 2 and R.mat_mul(t, G, p) == [[1, 0], [0, 1]]


def test_block_horner_equals_the_sum_of_powers():
    p, n, b, k = 65521, 6, 2, 2
    rng = np.random.default_rng(3)
    M = rng.integers(0, p, size=(n, n)).tolist()
    V = rng.integers(0, p, size=(n, b)).tolist()
    Cs = rng.integers(0, p, size=(4, b, k)).tolist()
    want = [[0] * k for _ in range(n)]
    P = V
    for Ct in Cs:
        want = [[(x + y) % p for x, y in zip(rx, ry)] for rx, ry in zip(want, R.mat_mul(P, Ct, p))]
        P = R.mat_mul(M, P, p)
    assert BS.block_poly_apply(M, Cs, V, p) == want


def ref_try0(S, M, B, b, p, seq_numpy=False):
    n = M.n
    U, Z = S.minpoly_vectors(n, b, K.SEED, p)
    Bl = [[int(x) % p for x in row] for row in np.asarray(B).reshape(n, -1)]
    seq = None
    if seq_numpy:
        V = np.array(Z, dtype=np.int64)
        V[:, : len(Bl[0])] = np.array(Bl, dtype=np.int64)
        seq = [[[int(x) for x in row] for row in T] for T in K.np_block_sequence(M, U, V, K.terms(n, b), p)]
    return BS.solve_try(K.dense_of(M), Bl, [[int(x) % p for x in r] for r in U], [[int(x) % p for x in r] for r in Z], p, seq=seq)


@pytest.mark.parametrize("trans", (False, True))
@pytest.mark.parametrize("n,b,k", K.SHAPES)
@pytest.mark.parametrize("p", (K.P16, K.P32))
def test_the_reference_decides_the_gpu_cases_at_try_0(S, p, n, b, k, trans):
    M, B = K.system(n, k, p)
    if trans:   # x A = b is A^T x = b
        M = M.transpose()
    X, status, info = ref_try0(S, M, B, b, p)
    assert status == [1] * k, info
    D = K.dense_of(M)
    for j in range(k):   # A x = b, directly, and x is the unique solution
        col = [X[r][j] for r in range(n)]
        assert [sum(a * x for a, x in zip(row, col)) % p for row in D] == [int(B[r, j]) % p for r in range(n)]
        assert col == BS.solve_dense(D, [int(B[r, j]) for r in range(n)], p)
    # the numpy products the GPU tests lean on give the same sequence as the integers
    X2, status2, _ = ref_try0(S, M, B, b, p, seq_numpy=True)
    assert (X2, status2) == (X, status)


@pytest.mark.parametrize("p", (K.P16, K.P32))
def test_the_reference_on_the_planted_singular_matrix(S, p):
    n, b = K.SINGULAR
    M, B = K.system(n, 2, p, kind="singular")
    D = K.dense_of(M)
    assert R.rank_mod(D, p) == n - 1
    X, status, info = ref_try0(S, M, B, b, p)
    assert status == [1, 2], info
    c0, c1 = [X[r][0] for r in range(n)], [X[r][1] for r in range(n)]
    assert [sum(a * x for a, x in zip(row, c0)) % p for row in D] == [int(B[r, 0]) % p for r in range(n)]
    assert any(c1) and not any(sum(a * x for a, x in zip(row, c1)) % p for row in D)


@pytest.mark.parametrize("n,b,k", K.MID)
def test_the_reference_decides_n_130_at_try_0(S, n, b, k):
    p = K.P16
    M, B = K.system(n, k, p)
    X, status, info = ref_try0(S, M, B, b, p, seq_numpy=True)
    assert status == [1] * k, info
    assert all(K.residual_is_zero(M, np.array(X, dtype=np.int64), B, p))


@pytest.mark.parametrize("kind,b,k", K.SPECIAL)
@pytest.mark.parametrize("p", (K.P16, K.P32))
def test_the_reference_decides_the_identity_and_a_permutation_by_the_residual(S, p, kind, b, k):
    M, B = K.special(kind, k, p)
    X, status, info = ref_try0(S, M, B, b, p)
    assert status == [1] * k, info
    if (kind, b) != ("permutation", 16):
        assert sum(info["rowdeg"]) < M.n   # the degrees do not reach n: only the residual says that x is right
    assert all(K.residual_is_zero(M, np.array(X, dtype=np.int64), B, p))
