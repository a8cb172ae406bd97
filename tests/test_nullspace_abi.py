"""CPU tests of the kernel-basis boundary (spasm_amd_dense_column_echelon, _block_precond_sequence, _wiedemann_kernel*,
_wiedemann_kernel_stats): symbols and bindings, the refusals that come before anything touches a device, the empty inputs that need
none, and the Python restatement (tests/nullspace_ref.py) run on the inputs of tests/test_gpu_wiedemann_kernel.py
(tests/nullspace_cases.py) with the seeded draws of the device: it completes every one of them within 3 tries, so the GPU test may
ask the device for the same.  Nothing here needs a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import block_wiedemann_ref as R
import nullspace_cases as K
import nullspace_ref as NS

SENTINEL = 0x5A5A5A5A
SYMBOLS = [
    "spasm_amd_dense_column_echelon", "spasm_amd_block_precond_sequence", "spasm_amd_wiedemann_kernel",
    "spasm_amd_spmv_wiedemann_kernel", "spasm_amd_dcsr_wiedemann_kernel", "spasm_amd_wiedemann_kernel_stats",
]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spasm_amd.h")


def test_kernel_symbols_exported_with_the_documented_signatures(S):
    lib = S._abi.lib()
    for name in SYMBOLS:
        assert name in S._abi.SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.restype == S._abi.SIGNATURES[name][0] and fn.argtypes == S._abi.SIGNATURES[name][1], name
    for name in ("column_echelon", "block_precond_sequence", "wiedemann_kernel", "wiedemann_kernel_stats"):
        assert callable(getattr(S, name)), name
        assert name in S.__all__, name
    assert callable(S.SpMV.block_precond_sequence) and callable(S.SpMV.wiedemann_kernel) and callable(S.DeviceCSR.wiedemann_kernel)
    assert len(S.api.WIEDEMANN_KERNEL_STATS) == len(set(S.api.WIEDEMANN_KERNEL_STATS)) == 19
    assert len(S.api.BLOCK_SOLVE_STATS) == 16 and len(S.api.BLOCK_STATS) == 10   # the neighbours keep their slots
    hdr = open(HEADER).read()
    for decl in (
        "int spasm_amd_dense_column_echelon(i64 rows, int K, spasm_ZZp *X, i64 ldx, i64 prime, int *rank, int *pivots);",
        "int spasm_amd_block_precond_sequence(spasm_amd_spmv *op, int trans, int b, int len, const spasm_ZZp *d_left, const spasm_ZZp *d_right",
        "int spasm_amd_wiedemann_kernel(const struct spasm_csr *A, int trans, int b, int want, uint64_t seed, int tries, int certify,",
        "int spasm_amd_spmv_wiedemann_kernel(spasm_amd_spmv *op, int trans, int b, int want, uint64_t seed, int tries, int certify,",
        "int spasm_amd_dcsr_wiedemann_kernel(const spasm_amd_dcsr *D, int trans, int b, int want, uint64_t seed, int tries, int certify,",
        "void spasm_amd_wiedemann_kernel_stats(i64 *out);",
        "THIS IS A PROOF",
        "EVERY RETURNED COLUMN IS A PROVED",
    ):
        assert decl in hdr, decl


def test_column_echelon_refusals_come_before_any_device(S):
    lib = S._abi.lib()
    err = S._abi.last_error
    who = "spasm_amd_dense_column_echelon"
    X = (C.c_int32 * 256)(*([SENTINEL] * 256))
    piv = (C.c_int32 * 64)(*([-7] * 64))
    rank = C.c_int32(-7)
    ech = lambda rows, k, x, ld, p, r, pv: lib.spasm_amd_dense_column_echelon(rows, k, x, ld, p, r, pv)
    for k in (-1, 65, 1000):
        assert ech(2, k, X, 1000, 65521, C.byref(rank), piv) == -1 and err() == f"{who}: K out of range (0 <= K <= 64)"
    assert ech(2, 3, X, 2, 65521, C.byref(rank), piv) == -1 and err() == f"{who}: ldx < K"
    for rows in (-1, 2**30, 2**40):
        assert ech(rows, 3, X, 3, 65521, C.byref(rank), piv) == -1 and err() == f"{who}: rows out of range (0 <= rows < 2^30)"
    for p in (0, 1, 2, 0xFFFFFFFC, 2**40):
        assert ech(2, 3, X, 3, p, C.byref(rank), piv) == -1 and err() == f"{who}: prime out of range (2 < p <= 0xfffffffb)"
    assert ech(2, 3, None, 3, 65521, C.byref(rank), piv) == -1 and err() == f"{who}: NULL array"
    assert ech(2, 3, X, 3, 65521, None, piv) == -1 and err() == f"{who}: NULL array"
    assert ech(2, 3, X, 3, 65521, C.byref(rank), None) == -1 and err() == f"{who}: NULL array"
    assert list(X) == [SENTINEL] * 256 and list(piv) == [-7] * 64 and rank.value == -7
    with pytest.raises(TypeError):
        S.column_echelon(np.zeros((2, 2)), 65521)
    with pytest.raises(S.SpasmError, match=r"K out of range \(0 <= K <= 64\)"):
        S.column_echelon(np.zeros((2, 65), dtype=np.int32), 65521)


def test_kernel_refusals_come_before_any_device(S):
    lib = S._abi.lib()
    err = S._abi.last_error
    who = "spasm_amd_wiedemann_kernel"
    A = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)], []], 2, prime=127)
    N = (C.c_int32 * 256)(*([SENTINEL] * 256))
    piv = (C.c_int32 * 64)(*([-7] * 64))
    found, complete = C.c_int32(-7), C.c_int32(-7)
    f, c = C.byref(found), C.byref(complete)
    ker = lib.spasm_amd_wiedemann_kernel
    for name in ("spasm_amd_wiedemann_kernel", "spasm_amd_dcsr_wiedemann_kernel"):
        assert getattr(lib, name)(None, 0, 2, 1, 0, 3, 0, N, 1, f, piv, c) == -1 and err() == f"{name}: NULL matrix"
    assert lib.spasm_amd_spmv_wiedemann_kernel(None, 0, 2, 1, 0, 3, 0, N, 1, f, piv, c) == -1
    assert err() == "spasm_amd_spmv_wiedemann_kernel: NULL operator"
    assert lib.spasm_amd_block_precond_sequence(None, 0, 2, 1, N, None, N, 2, N, 2, N) == -1
    assert err() == "spasm_amd_block_precond_sequence: NULL operator"
    for b in (0, 1, 3, 5, 12, 32, -2):
        assert ker(A.data, 0, b, 1, 0, 3, 0, N, 1, f, piv, c) == -1 and err() == f"{who}: b must be 2, 4, 8 or 16"
    for tr in (-1, 2):
        assert ker(A.data, tr, 2, 1, 0, 3, 0, N, 1, f, piv, c) == -1 and err() == f"{who}: trans must be 0 or 1"
    for want in (-1, 65):
        assert ker(A.data, 0, 2, want, 0, 3, 0, N, 100, f, piv, c) == -1 and err() == f"{who}: want out of range (0 <= want <= 64)"
    assert ker(A.data, 0, 2, 4, 0, 3, 0, N, 3, f, piv, c) == -1 and err() == f"{who}: ldn < want"
    for tries in (0, -1):
        assert ker(A.data, 0, 2, 1, 0, tries, 0, N, 1, f, piv, c) == -1 and err() == f"{who}: tries < 1"
    assert ker(A.data, 0, 2, 1, 0, 3, 0, None, 1, f, piv, c) == -1 and err() == f"{who}: NULL array"
    assert ker(A.data, 0, 2, 1, 0, 3, 0, N, 1, None, piv, c) == -1 and err() == f"{who}: NULL array"
    assert ker(A.data, 0, 2, 1, 0, 3, 0, N, 1, f, None, c) == -1 and err() == f"{who}: NULL array"
    assert ker(A.data, 0, 2, 1, 0, 3, 0, N, 1, f, piv, None) == -1 and err() == f"{who}: NULL array"
    assert list(N) == [SENTINEL] * 256 and list(piv) == [-7] * 64 and (found.value, complete.value) == (-7, -7)
    with pytest.raises(S.SpasmError, match="b must be 2, 4, 8 or 16"):
        S.wiedemann_kernel(A, b=3)
    with pytest.raises(S.SpasmError, match="tries < 1"):
        S.wiedemann_kernel(A, want=1, b=2, tries=0)
    with pytest.raises(TypeError):
        S.wiedemann_kernel(np.zeros((2, 2)))
    with pytest.raises(TypeError):
        S.block_precond_sequence(None, np.zeros((2, 2), dtype=np.int32), np.zeros((2, 2), dtype=np.int32), 3, np.ones(2, dtype=np.int32))
    # the header documents every refusal, the ones that need a resident operator among them
    doc = " ".join(open(HEADER).read().split())
    doc = doc[doc.index("---- kernel bases without fill-in"):]
    for words in ('"K out of range (0 <= K <= 64)"', '"ldx < K"', '"rows out of range (0 <= rows < 2^30)"', '"b must be 2, 4, 8 or 16"',
                  '"trans must be 0 or 1"', '"want out of range (0 <= want <= 64)"', '"ldn < want"', '"tries < 1"',
                  '"len out of range (1 <= len < 2^24)"', '"bad arguments (trans 0/1, ldu >= b, ldv >= b)"',
                  '"Wiedemann kernel limited to dim < 2^24"', '"no HIP device"'):
        assert words in doc, words


def test_the_empty_inputs_need_no_device(S):
    E, piv = S.column_echelon(np.zeros((0, 5), dtype=np.int32), 65521)
    assert E.shape == (0, 5) and len(piv) == 0
    E, piv = S.column_echelon(np.zeros((7, 0), dtype=np.int32), 65521)
    assert E.shape == (7, 0) and len(piv) == 0
    assert S._abi.last_error() == ""
    for certify in (False, True):
        A = S.CSR.from_rows([[], [], []], 0, prime=65521)          # 3 x 0: dim = 0
        N, piv, complete = S.wiedemann_kernel(A, b=4, certify=certify)
        assert N.shape == (0, 0) and len(piv) == 0 and complete is True
        N, piv, complete = S.wiedemann_kernel(S.CSR.from_rows([], 3, prime=65521), b=4, trans=True, certify=certify)   # x A, A 0 x 3
        assert N.shape == (0, 0) and complete is True
        # a matrix without rows: the whole space, unit vectors, complete only as a certified answer
        N, piv, complete = S.wiedemann_kernel(S.CSR.from_rows([], 3, prime=65521), b=2, certify=certify)
        assert N.tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1]] and piv.tolist() == [0, 1, 2] and complete is certify
        N, piv, complete = S.wiedemann_kernel(S.CSR.from_rows([], 3, prime=65521), want=2, b=2, certify=certify)
        assert N.tolist() == [[1, 0], [0, 1], [0, 0]] and piv.tolist() == [0, 1] and complete is False
    assert S._abi.last_error() == ""
    st = S.wiedemann_kernel_stats()
    assert (st["n"], st["m"], st["b"], st["want"], st["found"], st["products"], st["tries"]) == (0, 3, 2, 2, 2, 0, 0)


def test_kernel_fails_loudly_without_gpu(S):
    if S._abi.lib().spasm_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    A = S.CSR.from_rows([[(0, 1), (1, 2)], [(0, 2), (1, 4)]], 2, prime=127)
    with pytest.raises(S.SpasmError, match="no HIP device"):
        S.wiedemann_kernel(A, b=2)
    X = np.full((2, 2), SENTINEL, dtype=np.int32)
    piv = np.full(2, -7, dtype=np.int32)
    rank = C.c_int32(-7)
    assert S._abi.lib().spasm_amd_dense_column_echelon(2, 2, X.ctypes.data, 2, 127, C.byref(rank), piv.ctypes.data) == -1
    assert S._abi.last_error().startswith("spasm_amd_dense_column_echelon") and "no HIP device" in S._abi.last_error()
    assert (X == SENTINEL).all() and (piv == -7).all() and rank.value == -7


# ---------------------------------------------------------------- the reference on itself
def independent_rref(M, p):
    """Gauss-Jordan that picks the LAST eligible row as pivot and normalizes at the end: another route to the same unique form"""
    M = [[x % p for x in row] for row in M]
    rank, cols = 0, len(M[0])
    for c in range(cols):
        cand = [r for r in range(rank, len(M)) if M[r][c]]
        if not cand:
            continue
        M[cand[-1]], M[rank] = M[rank], M[cand[-1]]
        for r in range(len(M)):
            if r != rank and M[r][c]:
                f = M[r][c] * pow(M[rank][c], p - 2, p) % p
                M[r] = [(x - f * y) % p for x, y in zip(M[r], M[rank])]
        rank += 1
    out = []
    for row in M[:rank]:
        lead = next(x for x in row if x)
        out.append([x * pow(lead, p - 2, p) % p for x in row])
    return out


@pytest.mark.parametrize("p", (3, 65521, 4294967291))
def test_the_python_echelon_form_is_the_transpose_of_an_independent_rref(p):
    rng = np.random.default_rng(p % 1009)
    for rows, k, rank in ((9, 4, 4), (9, 5, 3), (3, 6, 3), (12, 7, 0), (1, 1, 1), (40, 17, 11)):
        base = rng.integers(0, p, size=(rows, max(rank, 1)))
        X = (base @ rng.integers(0, p, size=(max(rank, 1), k)).astype(object)) % p if rank else np.zeros((rows, k), dtype=object)
        X = [[int(x) for x in row] for row in np.asarray(X, dtype=object)]
        E, piv = NS.column_echelon(X, p)
        Rr = independent_rref([list(col) for col in zip(*X)], p)
        assert [list(col) for col in zip(*E)][: len(piv)] == Rr and len(Rr) == len(piv)
        assert all(not any(row[len(piv):]) for row in E)
        assert piv == sorted(set(piv)) and all(E[r][j] == 1 and sum(1 for x in E[r] if x) == 1 for j, r in enumerate(piv))
        assert all(not any(E[r][j] for r in range(piv[j])) for j in range(len(piv)))
        # the numpy route gives the same words
        En, pn = NS.np_column_echelon(np.array(X, dtype=object).astype(np.int64) if p < 2**31 else np.array(X, dtype=np.int64), p)
        assert pn == piv and (En.astype(np.int64) % p).tolist() == E
        # a column permutation and an invertible column operation leave the form alone
        perm = rng.permutation(k)
        assert NS.column_echelon([[row[c] for c in perm] for row in X], p) == (E, piv)


def test_the_nullspace_by_elimination_annihilates_and_has_the_right_size():
    p = 65521
    B = K.dense_of(K.matrix("tall40x30", p))
    N = NS.nullspace(B, 30, p)
    assert len(N[0]) == 5 == 30 - R.rank_mod(B, p)
    assert not any(any(row) for row in R.mat_mul(B, N, p))
    E, piv = NS.kernel_basis(B, 30, p)
    assert len(piv) == 5 and not any(any(row) for row in R.mat_mul(B, E, p))


@pytest.mark.parametrize("name,b,trans,nullity", K.CASES)
@pytest.mark.parametrize("p", K.PRIMES)
def test_the_reference_completes_the_gpu_cases_within_3_tries(S, p, name, b, trans, nullity):
    M = K.operand(name, p, trans)
    B = K.dense_of(M)
    nr, dim = M.n, M.m
    assert dim - R.rank_mod(B, p) == nullity
    seed = K.seed_of(name, b, trans, p)
    E, piv, complete, info = NS.kernel(B, dim, b, p, K.draws(S, nr, dim, b, seed, p), tries=K.TRIES, target=nullity)
    print(name, b, trans, p, info)
    assert complete and len(piv) == nullity, info
    want = NS.kernel_basis(B, dim, p)
    assert (E, piv) == want
    assert info["accepted"] - info["dependent"] == nullity
    if name == "wide20x33" and not trans:
        assert info["tries"] > 1   # 13 > b: more than one try is needed


def test_at_most_one_case_in_four_carries_another_seed():
    assert 4 * len(K.SEEDS) <= len(K.CASES) * len(K.PRIMES)
    assert all(k[:3] in {c[:3] for c in K.CASES} and k[3] in K.PRIMES for k in K.SEEDS)
