"""CPU tests of the matrix-algebra boundary (spasm_submatrix, spasm_amd_dcsr_*, spasm_amd_csr_mul / _lincomb, the operators of CSR
and DeviceCSR): symbols, bindings, the host-side submatrix entry for entry, and the argument checks that happen in Python before
any C call.  Nothing here needs a GPU."""
import numpy as np
import pytest

ALGEBRA_SYMBOLS = [
    "spasm_submatrix",
    "spasm_amd_dcsr_upload",
    "spasm_amd_dcsr_download",
    "spasm_amd_dcsr_info",
    "spasm_amd_dcsr_free",
    "spasm_amd_dcsr_mul",
    "spasm_amd_dcsr_lincomb",
    "spasm_amd_dcsr_submatrix",
    "spasm_amd_dcsr_equal",
    "spasm_amd_dcsr_stats",
    "spasm_amd_csr_mul",
    "spasm_amd_csr_lincomb",
]

RANGES = [((0, 0), (0, 0)), ((3, 3), (0, 7)), ((0, 9), (4, 4)), ((2, 11), (5, 23)), ((0, 1), (0, 1)), ((7, 8), (29, 30)), ("all", "all")]


def rand_unsorted(S, n, m, p, rng, empty_every=3):
    """n x m, distinct columns per row in random (unsorted) order, every empty_every-th row empty, balanced non-zero values"""
    rows = []
    for i in range(n):
        cnt = 0 if i % empty_every == 0 else int(rng.integers(1, max(2, m // 2)))
        rows.append(rng.permutation(m)[:cnt])
    ptr = np.zeros(n + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    j = np.concatenate(rows).astype(np.int32) if n else np.zeros(0, np.int32)
    x = S.balanced(rng.integers(1, p, size=len(j)), p)
    return S.CSR.from_arrays(n, m, ptr, j, x, prime=p)


def stored_rows(A, with_values=True):
    """rows as lists of (column, value) in STORED order"""
    p, j = A.p, A.j
    out = []
    for i in range(A.n):
        lo, hi = int(p[i]), int(p[i + 1])
        out.append(list(zip(j[lo:hi].tolist(), A.x[lo:hi].tolist())) if with_values else j[lo:hi].tolist())
    return out


def test_algebra_symbols_exported_and_bound(S):
    lib = S._abi.lib()
    for name in ALGEBRA_SYMBOLS:
        assert name in S._abi.SIGNATURES, name
        assert getattr(lib, name).argtypes == S._abi.SIGNATURES[name][1], name
    assert callable(S.submatrix) and S.DeviceCSR is not None
    for op in ("__add__", "__sub__", "__neg__", "__mul__", "__rmul__", "__getitem__", "equals"):
        assert hasattr(S.CSR, op), op
    # `==` on CSR stays identity
    assert "__eq__" not in S.CSR.__dict__ and "__hash__" not in S.CSR.__dict__


@pytest.mark.parametrize("p", [127, 0xFFFFFFFB])
def test_submatrix_against_numpy_slicing(S, p):
    rng = np.random.default_rng(p % 1000)
    n, m = 11, 30
    A = rand_unsorted(S, n, m, p, rng)
    D = A.todense()
    for (rr, cc) in RANGES:
        r0, r1 = (0, n) if rr == "all" else rr
        c0, c1 = (0, m) if cc == "all" else cc
        for B in (S.submatrix(A, range(r0, r1), range(c0, c1)), A[r0:r1, c0:c1]):
            assert B.shape == (r1 - r0, c1 - c0) and B.prime == p
            assert np.array_equal(B.todense(), D[r0:r1, c0:c1]), (rr, cc)
            assert B.nzmax == S.nnz(B) == int(np.count_nonzero(D[r0:r1, c0:c1]))
            # stored order kept: the row of A filtered, columns renumbered
            want = [[(c - c0, v) for (c, v) in row if c0 <= c < c1] for row in stored_rows(A)[r0:r1]]
            assert stored_rows(B) == want
        P = S.submatrix(A, range(r0, r1), range(c0, c1), with_values=False)
        assert not P.data.contents.x  # NULL
        assert stored_rows(P, False) == [[c - c0 for (c, _) in row if c0 <= c < c1] for row in stored_rows(A)[r0:r1]]
    # `:` and open ends
    assert np.array_equal(A[:, 3:9].todense(), D[:, 3:9]) and np.array_equal(A[4:, :].todense(), D[4:, :])
    assert np.array_equal(A[:, :].todense(), D)


def test_submatrix_of_a_pattern_and_of_empty_matrices(S):
    rng = np.random.default_rng(1)
    A = rand_unsorted(S, 6, 8, 42013, rng)
    P = S.submatrix(A, range(0, 6), range(0, 8), with_values=False)
    with pytest.raises(S.SpasmError, match="without values"):
        S.submatrix(P, range(0, 2), range(0, 2), with_values=True)
    Q = S.submatrix(P, range(1, 5), range(2, 7), with_values=False)
    assert stored_rows(Q, False) == [[c - 2 for (c, _) in row if 2 <= c < 7] for row in stored_rows(A)[1:5]]
    E = S.CSR.from_arrays(0, 0, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), prime=127)
    assert S.submatrix(E, range(0, 0), range(0, 0)).shape == (0, 0)


@pytest.mark.parametrize("rows,cols", [(range(0, 12), range(0, 30)), (range(-1, 3), range(0, 30)), (range(0, 11), range(0, 31)), (range(5, 2), range(0, 30)),
                                       (range(0, 11), range(9, 4)), (range(0, 11), range(-2, 4))])
def test_submatrix_ranges_outside_or_inverted(S, rows, cols):
    A = rand_unsorted(S, 11, 30, 127, np.random.default_rng(2))
    with pytest.raises(S.SpasmError, match="spasm_submatrix"):
        S.submatrix(A, rows, cols)
    assert S._abi.last_error() != ""
    S.submatrix(A, range(0, 1), range(0, 1))
    assert S._abi.last_error() == ""  # cleared by a success


def test_slices_with_a_step_and_other_keys_rejected(S):
    A = rand_unsorted(S, 11, 30, 127, np.random.default_rng(3))
    with pytest.raises(ValueError):
        A[0:10:2, :]
    with pytest.raises(ValueError):
        A[:, ::3]
    with pytest.raises(ValueError):
        S.submatrix(A, range(0, 10, 2), range(0, 30))
    with pytest.raises(TypeError):
        A[3]
    with pytest.raises(TypeError):
        A[1, 2]


def no_c_call(S, monkeypatch):
    """any matrix-algebra entry of the library that is reached fails the test"""
    class Trap:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            if name in ALGEBRA_SYMBOLS:
                raise AssertionError(f"{name} reached")
            return getattr(self._lib, name)

    real = S._abi.lib()
    monkeypatch.setattr(S._abi, "lib", lambda: Trap(real))


def test_mismatches_rejected_in_python_before_any_c_call(S, monkeypatch):
    rng = np.random.default_rng(4)
    A = rand_unsorted(S, 5, 7, 127, rng)
    B = rand_unsorted(S, 6, 4, 127, rng)       # inner dimension differs from A.m
    C7 = rand_unsorted(S, 7, 4, 65521, rng)    # fits, other prime
    A2 = rand_unsorted(S, 5, 7, 65521, rng)
    A3 = rand_unsorted(S, 5, 8, 127, rng)
    no_c_call(S, monkeypatch)
    for call in (lambda: A @ B, lambda: A @ C7, lambda: A + A2, lambda: A - A3, lambda: A + A3):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: 2.0 * A, lambda: A * 0.5, lambda: A * "3", lambda: A + 1, lambda: A - np.zeros((5, 7), np.int64), lambda: A * True,
                 lambda: A.equals(np.zeros((5, 7)))):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(ValueError):
        A * 2**64
    assert A.equals(A3) is False and A.equals(A2) is False  # shape / prime decide without the device


def test_csr_matmul_dispatch(S, monkeypatch):
    """A @ CSR reaches the product of matrices, A @ ndarray and ndarray @ A still reach _product"""
    seen = []
    monkeypatch.setattr(S.api, "_product", lambda A, x, trans: seen.append(("vec", trans)) or "v")
    monkeypatch.setattr(S.api, "_csr_mul", lambda A, B: seen.append(("mat", A.shape, B.shape)) or "m")
    monkeypatch.setattr(S.api, "_csr_lincomb", lambda a, A, b, B: seen.append(("lin", a, b, B is not None)) or "l")
    A = S.CSR(np.array([[1, 2, 0], [3, 6, 5]]))  # stored transpose: 3 x 2
    B = S.CSR.from_rows([[(0, 1)], [(2, 5)]], 3)  # 2 x 3
    assert A @ B == "m" and A @ np.arange(2) == "v" and np.arange(3) @ A == "v"
    assert A + A == "l" and A - A == "l" and -A == "l" and 3 * A == "l" and A * np.int64(-2) == "l"
    assert seen == [("mat", (3, 2), (2, 3)), ("vec", False), ("vec", True), ("lin", 1, 1, True), ("lin", 1, -1, True), ("lin", -1, 0, False), ("lin", 3, 0, False),
                    ("lin", -2, 0, False)]


def test_algebra_fails_loudly_without_gpu(S):
    if S._abi.lib().spasm_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    A = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)]], 2, prime=127)
    B = S.CSR.from_rows([[(1, 5)], [(0, 7), (1, 1)]], 2, prime=127)
    before = (stored_rows(A), stored_rows(B))
    for call in (lambda: A @ B, lambda: A + B, lambda: A - B, lambda: -A, lambda: 5 * A, lambda: S.DeviceCSR(A), lambda: A.equals(B)):
        with pytest.raises(S.SpasmError, match="no HIP device"):
            call()
    assert (stored_rows(A), stored_rows(B)) == before
    lib = S._abi.lib()
    assert not lib.spasm_amd_csr_mul(A.data, B.data) and "no HIP device" in S._abi.last_error()
    assert not lib.spasm_amd_dcsr_upload(A.data) and "no HIP device" in S._abi.last_error()
    # NULL handles are refused, not dereferenced
    assert not lib.spasm_amd_dcsr_mul(None, None) and S._abi.last_error() != ""
    assert lib.spasm_amd_dcsr_equal(None, None) < 0
    assert not lib.spasm_amd_dcsr_download(None)
    lib.spasm_amd_dcsr_free(None)
    # the host-side submatrix needs no device
    assert np.array_equal(A[0:1, 1:2].todense(), A.todense()[0:1, 1:2])
