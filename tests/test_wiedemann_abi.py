"""CPU tests of the boundary of spasm_amd_poly_apply / _poly_apply_dev / _wiedemann_solve / _spmv_wiedemann_solve /
_dcsr_wiedemann_solve / _wiedemann_stats: symbols and bindings, and the argument checks that come before anything touches a device
(for a host matrix all of them; an operator or a resident matrix needs a device to exist, so only their NULL handle is seen here
and the rest of their checks in the GPU files).  Nothing here needs a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

SENTINEL = 0x5A5A5A5A
SYMBOLS = [
    "spasm_amd_poly_apply", "spasm_amd_poly_apply_dev", "spasm_amd_wiedemann_solve", "spasm_amd_spmv_wiedemann_solve",
    "spasm_amd_dcsr_wiedemann_solve", "spasm_amd_wiedemann_stats",
]


def test_symbols_exported_with_the_documented_signatures(S):
    lib = S._abi.lib()
    for name in SYMBOLS:
        assert name in S._abi.SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.restype == S._abi.SIGNATURES[name][0] and fn.argtypes == S._abi.SIGNATURES[name][1], name
    for name in ("poly_apply", "wiedemann_solve", "wiedemann_stats"):
        assert callable(getattr(S, name)), name
        assert name in S.__all__, name
    assert callable(S.SpMV.poly_apply) and callable(S.SpMV.wiedemann_solve) and callable(S.DeviceCSR.wiedemann_solve)
    assert len(S.api.WIEDEMANN_STATS) == 10 and len(set(S.api.WIEDEMANN_STATS)) == 10
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spasm_amd.h")).read()
    hdr = " ".join(hdr.split())
    for decl in (
        "int spasm_amd_poly_apply(spasm_amd_spmv *op, int trans, int K, const int *deg, const spasm_ZZp *coef, i64 ldc, const spasm_ZZp *V, i64 ldv, "
        "spasm_ZZp *X, i64 ldx);",
        "int spasm_amd_poly_apply_dev(spasm_amd_spmv *op, int trans, int K, const int *deg, const spasm_ZZp *coef, i64 ldc, const spasm_ZZp *V, i64 ldv, "
        "spasm_ZZp *X, i64 ldx, void *stream);",
        "int spasm_amd_wiedemann_solve(const struct spasm_csr *A, int trans, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries, int maxdeg, "
        "const spasm_ZZp *U, spasm_ZZp *X, i64 ldx, int *status);",
        "int spasm_amd_spmv_wiedemann_solve(spasm_amd_spmv *op, int trans, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries, int maxdeg, "
        "const spasm_ZZp *U, spasm_ZZp *X, i64 ldx, int *status);",
        "int spasm_amd_dcsr_wiedemann_solve(const spasm_amd_dcsr *D, int trans, int K, const spasm_ZZp *B, i64 ldb, uint64_t seed, int tries, int maxdeg, "
        "const spasm_ZZp *U, spasm_ZZp *X, i64 ldx, int *status);",
        "void spasm_amd_wiedemann_stats(i64 *out);",
    ):
        assert decl in hdr, decl


class Buffers:
    """B, X and status with a sentinel in every word: a refused call must leave them as they are"""

    def __init__(self, words=16):
        self.B = (C.c_int32 * words)(*([1] * words))
        self.X = (C.c_int32 * words)(*([SENTINEL] * words))
        self.status = (C.c_int32 * words)(*([SENTINEL] * words))
        self.words = words

    def untouched(self):
        return list(self.X) == [SENTINEL] * self.words and list(self.status) == [SENTINEL] * self.words


def test_solve_argument_errors_come_before_any_device(S):
    lib = S._abi.lib()
    err = S._abi.last_error
    fn = lib.spasm_amd_wiedemann_solve
    b = Buffers()
    sq = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)]], 2, prime=127)
    call = lambda A, trans=0, K=2, B=b.B, ldb=2, U=None, X=b.X, ldx=2, status=b.status: fn(A, trans, K, B, ldb, 0, 3, 0, U, X, ldx, status)

    # NULL handles and arrays
    assert call(None) == -1 and err() == "spasm_amd_wiedemann_solve: NULL matrix"
    assert lib.spasm_amd_spmv_wiedemann_solve(None, 0, 2, b.B, 2, 0, 3, 0, None, b.X, 2, b.status) == -1
    assert err() == "spasm_amd_spmv_wiedemann_solve: NULL operator"
    assert lib.spasm_amd_dcsr_wiedemann_solve(None, 0, 2, b.B, 2, 0, 3, 0, None, b.X, 2, b.status) == -1
    assert err() == "spasm_amd_dcsr_wiedemann_solve: NULL matrix"
    assert call(sq.data, B=None) == -1 and err() == "spasm_amd_wiedemann_solve: NULL array"
    assert call(sq.data, X=None) == -1 and err() == "spasm_amd_wiedemann_solve: NULL array"
    assert call(sq.data, status=None) == -1 and err() == "spasm_amd_wiedemann_solve: NULL array"
    assert b.untouched()

    # a matrix that is not square
    tall = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)], []], 2, prime=127)
    assert call(tall.data) == -1 and err() == "spasm_amd_wiedemann_solve: not square (3 x 2)"
    with pytest.raises(S.SpasmError, match=r"spasm_amd_wiedemann_solve: not square \(3 x 2\)"):
        S.wiedemann_solve(tall, np.zeros((3, 2), dtype=np.int32))

    # K outside 1 .. 64, trans, leading dimensions
    for K in (0, -1, 65):
        assert call(sq.data, K=K, ldb=65, ldx=65) == -1 and err() == "spasm_amd_wiedemann_solve: K out of range (1 <= K <= 64)", K
    assert call(sq.data, trans=2) == -1 and err() == "spasm_amd_wiedemann_solve: trans must be 0 or 1"
    assert call(sq.data, ldb=1) == -1 and err() == "spasm_amd_wiedemann_solve: ldb < K"
    assert call(sq.data, ldx=1) == -1 and err() == "spasm_amd_wiedemann_solve: ldx < K"
    assert b.untouched()

    # a prime outside 3 .. 0xFFFFFFFB
    bad = S.CSR.from_rows([[(0, 1)], [(1, 1)]], 2, prime=127)
    for prime in (2, 1, 0xFFFFFFFC, 4294967311):
        bad.data.contents.field.p = prime
        assert call(bad.data) == -1 and err() == "spasm_amd_wiedemann_solve: prime out of range (2 < p <= 0xfffffffb)", prime
    bad.data.contents.field.p = 127
    assert b.untouched()

    # n >= 2^24: no entry is needed to see it
    n = 1 << 24
    huge = S.CSR.from_arrays(n, n, np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), prime=127)
    assert call(huge.data, K=1, ldb=1, ldx=1) == -1 and err() == "spasm_amd_wiedemann_solve: Wiedemann solve limited to n < 2^24"
    assert b.untouched()


def test_poly_apply_null_operator(S):
    lib = S._abi.lib()
    b = Buffers()
    deg = (C.c_int32 * 2)(1, 1)
    assert lib.spasm_amd_poly_apply(None, 0, 2, deg, b.B, 2, b.B, 2, b.X, 2) == -1
    assert S._abi.last_error() == "spasm_amd_poly_apply: NULL operator"
    assert lib.spasm_amd_poly_apply_dev(None, 0, 2, deg, b.B, 2, b.B, 2, b.X, 2, None) == -1
    assert S._abi.last_error() == "spasm_amd_poly_apply_dev: NULL operator"
    assert b.untouched()
    with pytest.raises(TypeError, match="an SpMV operator expected"):
        S.poly_apply(None, [[1]], np.zeros((2, 1), dtype=np.int32))


def test_the_system_without_unknowns_and_the_stats_cleared_by_every_call(S):
    E = S.CSR.from_rows([], 0, prime=65521)
    X, status = S.wiedemann_solve(E, np.zeros((0, 3), dtype=np.int32))
    assert X.shape == (0, 3) and status.tolist() == [1, 1, 1] and S._abi.last_error() == ""
    st = S.wiedemann_stats()
    assert list(st) == list(S.api.WIEDEMANN_STATS)
    assert (st["n"], st["K"], st["solved"], st["products"], st["launches"]) == (0, 3, 3, 0, 0)
    # a refused call clears them
    tall = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)], []], 2, prime=127)
    with pytest.raises(S.SpasmError):
        S.wiedemann_solve(tall, np.zeros((3, 1), dtype=np.int32))
    assert not any(S.wiedemann_stats().values())
    # and so does a call of the other family member
    S.wiedemann_solve(E, np.zeros((0, 2), dtype=np.int32))
    assert S.wiedemann_stats()["K"] == 2
    assert S._abi.lib().spasm_amd_poly_apply(None, 0, 1, None, None, 1, None, 1, None, 1) == -1
    assert not any(S.wiedemann_stats().values())
