"""CPU tests of the characteristic-polynomial boundary (spasm_amd_charpoly_batch / _charpoly / _dcsr_charpoly / _charpoly_stats):
symbols, bindings, the argument checks -- which come before anything touches a device and leave the output slots as they were --
and the loud failure without a GPU.  Nothing here needs one."""
import ctypes as C
import os

import numpy as np
import pytest

CHARPOLY_SYMBOLS = ["spasm_amd_charpoly_batch", "spasm_amd_charpoly", "spasm_amd_dcsr_charpoly", "spasm_amd_charpoly_stats"]
SENTINEL = 0x5A5A5A5A
SLOT = 4   # words per output slot of the small matrices below (n + 1 = 3 are needed)


def square(S, prime=127):
    return S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)]], 2, prime=prime)


def tall(S, prime=127):
    return S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)], []], 2, prime=prime)


def too_large(S, prime=127):
    """1025 x 1025 with one entry: over the limit of the global path"""
    return S.CSR.from_rows([[(0, 1)]] + [[] for _ in range(1024)], 1025, prime=prime)


def csr_array(S, mats):
    return (C.POINTER(S._abi.CsrStruct) * max(len(mats), 1))(*[A.data if A is not None else None for A in mats])


def sentinel_slots(count, words=SLOT):
    """count output slots filled with a sentinel, the array of pointers to them, and a check that none was written"""
    bufs = [(C.c_int32 * words)(*([SENTINEL] * words)) for _ in range(count)]
    ptrs = (C.POINTER(C.c_int32) * max(count, 1))(*[C.cast(b, C.POINTER(C.c_int32)) for b in bufs])
    return bufs, ptrs, lambda: all(b[i] == SENTINEL for b in bufs for i in range(words))


def test_charpoly_symbols_exported_with_the_documented_signatures(S):
    lib = S._abi.lib()
    P = C.POINTER
    want = {
        "spasm_amd_charpoly_batch": (C.c_int32, [C.c_int32, P(P(S._abi.CsrStruct)), P(P(C.c_int32))]),
        "spasm_amd_charpoly": (C.c_int32, [P(S._abi.CsrStruct), P(C.c_int32)]),
        "spasm_amd_dcsr_charpoly": (C.c_int32, [C.c_void_p, P(C.c_int32)]),
        "spasm_amd_charpoly_stats": (None, [P(C.c_int64)]),
    }
    for name in CHARPOLY_SYMBOLS:
        assert name in S._abi.SIGNATURES, name
        assert S._abi.SIGNATURES[name] == want[name], name
        fn = getattr(lib, name)
        assert fn.restype == want[name][0] and fn.argtypes == want[name][1], name
    for name in ("charpoly", "charpoly_batch", "charpoly_stats"):
        assert callable(getattr(S, name)), name
        assert name in S.__all__, name
    assert callable(S.DeviceCSR.charpoly)
    assert len(S.api.CHARPOLY_STATS) == 8 and len(set(S.api.CHARPOLY_STATS)) == 8
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spasm_amd.h")).read()
    for decl in (
        "int spasm_amd_charpoly_batch(int count, const struct spasm_csr *const *A, spasm_ZZp *const *coef);",
        "int spasm_amd_charpoly(const struct spasm_csr *A, spasm_ZZp *coef);",
        "int spasm_amd_dcsr_charpoly(const spasm_amd_dcsr *D, spasm_ZZp *coef);",
        "void spasm_amd_charpoly_stats(i64 *out);",
    ):
        assert decl in hdr, decl


def test_charpoly_batch_argument_errors_return_minus_one_and_leave_the_slots(S):
    fn = S._abi.lib().spasm_amd_charpoly_batch
    A = square(S)
    bufs, out, untouched = sentinel_slots(3)
    # count < 0
    assert fn(-1, csr_array(S, [A]), out) == -1
    assert "count < 0" in S._abi.last_error() and "spasm_amd_charpoly_batch" in S._abi.last_error()
    # a NULL array (of matrices, of outputs)
    assert fn(2, None, out) == -1 and "NULL array" in S._abi.last_error()
    assert fn(2, csr_array(S, [A, A]), None) == -1 and "NULL array" in S._abi.last_error()
    # a NULL matrix: the index is named
    assert fn(3, csr_array(S, [A, None, A]), out) == -1
    assert "matrix 1" in S._abi.last_error() and "NULL matrix" in S._abi.last_error()
    # a NULL output slot: the index is named
    holed = (C.POINTER(C.c_int32) * 3)(out[0], out[1], None)
    assert fn(3, csr_array(S, [A, A, A]), holed) == -1
    assert "matrix 2" in S._abi.last_error() and "NULL array" in S._abi.last_error()
    # a matrix that is not square
    assert fn(3, csr_array(S, [A, A, tall(S)]), out) == -1
    assert "matrix 2: not square (3 x 2)" in S._abi.last_error()
    # a matrix over the limit of the global path (the slot is never written, so its size does not matter)
    assert fn(3, csr_array(S, [A, too_large(S), A]), out) == -1
    assert "matrix 1: characteristic polynomial limited to n <= 1024 (n = 1025)" in S._abi.last_error()
    # a prime out of range
    for bad in (2, 0xFFFFFFFB + 2):
        B = square(S)
        B.data.contents.field.p = bad
        assert fn(2, csr_array(S, [A, B]), out) == -1
        assert "matrix 1" in S._abi.last_error() and "prime out of range" in S._abi.last_error()
    # a column index outside the matrix
    B = square(S)
    for bad in (2, -1):
        B.j[2] = bad
        assert fn(2, csr_array(S, [A, B]), out) == -1
        assert "matrix 1" in S._abi.last_error() and "column index" in S._abi.last_error()
    # a matrix without values
    B = S.submatrix(A, range(0, 2), range(0, 2), with_values=False)
    assert fn(2, csr_array(S, [A, B]), out) == -1
    assert "matrix 1" in S._abi.last_error() and "x == NULL" in S._abi.last_error()
    assert untouched()


def test_single_matrix_argument_errors_return_minus_one_and_leave_the_slot(S):
    lib = S._abi.lib()
    bufs, _, untouched = sentinel_slots(1)
    out = C.cast(bufs[0], C.POINTER(C.c_int32))
    assert lib.spasm_amd_charpoly(None, out) == -1 and "spasm_amd_charpoly: NULL matrix" in S._abi.last_error()
    assert lib.spasm_amd_charpoly(square(S).data, None) == -1 and "NULL array" in S._abi.last_error()
    assert lib.spasm_amd_charpoly(tall(S).data, out) == -1 and "not square (3 x 2)" in S._abi.last_error()
    assert lib.spasm_amd_charpoly(too_large(S).data, out) == -1
    assert "characteristic polynomial limited to n <= 1024 (n = 1025)" in S._abi.last_error()
    B = square(S)
    B.j[2] = 2
    assert lib.spasm_amd_charpoly(B.data, out) == -1 and "column index" in S._abi.last_error()
    B = square(S)
    B.data.contents.field.p = 2
    assert lib.spasm_amd_charpoly(B.data, out) == -1 and "prime out of range" in S._abi.last_error()
    assert lib.spasm_amd_dcsr_charpoly(None, out) == -1 and "spasm_amd_dcsr_charpoly: NULL matrix" in S._abi.last_error()
    assert untouched()


def test_count_zero_succeeds_and_clears_the_error(S):
    fn = S._abi.lib().spasm_amd_charpoly_batch
    bufs, out, untouched = sentinel_slots(1)
    assert fn(-1, None, out) == -1 and S._abi.last_error() != ""
    assert fn(0, None, None) == 0
    assert S._abi.last_error() == ""
    assert fn(0, csr_array(S, []), out) == 0 and untouched()
    assert S.charpoly_stats() == dict.fromkeys(S.api.CHARPOLY_STATS, 0)
    assert S.charpoly_batch([]) == []


def test_python_wrappers_check_their_arguments(S):
    with pytest.raises(TypeError):
        S.charpoly_batch([square(S), np.zeros((2, 2), dtype=np.int64)])
    with pytest.raises(TypeError):
        S.charpoly(np.zeros((2, 2), dtype=np.int64))
    with pytest.raises(S.SpasmError, match=r"not square \(3 x 2\)"):
        S.charpoly(tall(S))
    with pytest.raises(S.SpasmError, match=r"matrix 1: not square \(3 x 2\)"):
        S.charpoly_batch([square(S), tall(S)])
    with pytest.raises(S.SpasmError, match=r"matrix 1: characteristic polynomial limited to n <= 1024 \(n = 1025\)"):
        S.charpoly_batch([square(S), too_large(S)])
    with pytest.raises(S.SpasmError, match=r"limited to n <= 1024 \(n = 1025\)"):
        S.charpoly(too_large(S))
    S._abi.lib().spasm_amd_charpoly_stats(None)  # ignored, not dereferenced


def test_charpoly_fails_loudly_without_gpu(S):
    if S._abi.lib().spasm_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    A, B = square(S), square(S, prime=65521)
    bufs, out, untouched = sentinel_slots(2)
    assert S._abi.lib().spasm_amd_charpoly_batch(2, csr_array(S, [A, B]), out) == -1
    assert "no HIP device" in S._abi.last_error()
    assert S._abi.lib().spasm_amd_charpoly(A.data, out[0]) == -1 and "no HIP device" in S._abi.last_error()
    assert untouched()
    with pytest.raises(S.SpasmError, match="no HIP device"):
        S.charpoly_batch([A, B])
    with pytest.raises(S.SpasmError, match="no HIP device"):
        S.charpoly(A)
