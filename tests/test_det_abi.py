"""CPU tests of the determinant boundary (spasm_amd_det_batch / _det / _blocks_det / _dcsr_det / _det_stats): symbols, bindings,
the argument checks -- which come before anything touches a device and leave the output slots as they were -- and the loud failure
without a GPU.  Nothing here needs one."""
import ctypes as C
import os

import numpy as np
import pytest

DET_SYMBOLS = ["spasm_amd_det_batch", "spasm_amd_det", "spasm_amd_blocks_det", "spasm_amd_dcsr_det", "spasm_amd_det_stats"]
SENTINEL = 0x5A5A5A5A


def square(S, prime=127):
    return S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)]], 2, prime=prime)


def tall(S, prime=127):
    return S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)], []], 2, prime=prime)


def csr_array(S, mats):
    return (C.POINTER(S._abi.CsrStruct) * max(len(mats), 1))(*[A.data if A is not None else None for A in mats])


def sentinel_slots(count):
    out = (C.c_int32 * count)(*([SENTINEL] * count))
    return out, lambda: all(out[i] == SENTINEL for i in range(count))


def test_det_symbols_exported_with_the_documented_signatures(S):
    lib = S._abi.lib()
    P = C.POINTER
    want = {
        "spasm_amd_det_batch": (C.c_int32, [C.c_int32, P(P(S._abi.CsrStruct)), P(C.c_int32)]),
        "spasm_amd_det": (C.c_int32, [P(S._abi.CsrStruct), P(C.c_int32)]),
        "spasm_amd_blocks_det": (C.c_int32, [C.c_void_p, P(C.c_int32)]),
        "spasm_amd_dcsr_det": (C.c_int32, [C.c_void_p, P(C.c_int32)]),
        "spasm_amd_det_stats": (None, [P(C.c_int64)]),
    }
    for name in DET_SYMBOLS:
        assert name in S._abi.SIGNATURES, name
        assert S._abi.SIGNATURES[name] == want[name], name
        fn = getattr(lib, name)
        assert fn.restype == want[name][0] and fn.argtypes == want[name][1], name
    for name in ("det", "det_batch", "det_stats"):
        assert callable(getattr(S, name)), name
    assert callable(S.DeviceCSR.det) and callable(S.DeviceBlocks.det) and callable(S.blocks.det)
    assert len(S.api.DET_STATS) == 8 and len(set(S.api.DET_STATS)) == 8
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spasm_amd.h")).read()
    for decl in (
        "int spasm_amd_det_batch(int count, const struct spasm_csr *const *A, spasm_ZZp *det);",
        "int spasm_amd_det(const struct spasm_csr *A, spasm_ZZp *det);",
        "int spasm_amd_blocks_det(spasm_amd_blocks *B, spasm_ZZp *det);",
        "int spasm_amd_dcsr_det(const spasm_amd_dcsr *D, spasm_ZZp *det);",
        "void spasm_amd_det_stats(i64 *out);",
    ):
        assert decl in hdr, decl


def test_det_batch_argument_errors_return_minus_one_and_leave_the_slots(S):
    fn = S._abi.lib().spasm_amd_det_batch
    A = square(S)
    out, untouched = sentinel_slots(3)
    # count < 0
    assert fn(-1, csr_array(S, [A]), out) == -1
    assert "count < 0" in S._abi.last_error() and "spasm_amd_det_batch" in S._abi.last_error()
    # a NULL array (of matrices, of outputs)
    assert fn(2, None, out) == -1 and "NULL array" in S._abi.last_error()
    assert fn(2, csr_array(S, [A, A]), None) == -1 and "NULL array" in S._abi.last_error()
    # a NULL matrix: the index is named
    assert fn(3, csr_array(S, [A, None, A]), out) == -1
    assert "matrix 1" in S._abi.last_error() and "NULL matrix" in S._abi.last_error()
    # a matrix that is not square
    assert fn(3, csr_array(S, [A, A, tall(S)]), out) == -1
    assert "matrix 2: not square (3 x 2)" in S._abi.last_error()
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
    assert untouched()


def test_whole_matrix_argument_errors_return_minus_one_and_leave_the_slot(S):
    lib = S._abi.lib()
    out, untouched = sentinel_slots(1)
    assert lib.spasm_amd_det(None, out) == -1 and "spasm_amd_det: NULL matrix" in S._abi.last_error()
    assert lib.spasm_amd_det(square(S).data, None) == -1 and "NULL array" in S._abi.last_error()
    assert lib.spasm_amd_det(tall(S).data, out) == -1 and "not square (3 x 2)" in S._abi.last_error()
    B = square(S)
    B.j[2] = 2
    assert lib.spasm_amd_det(B.data, out) == -1 and "column index" in S._abi.last_error()
    B = square(S)
    B.data.contents.field.p = 2
    assert lib.spasm_amd_det(B.data, out) == -1 and "prime out of range" in S._abi.last_error()
    assert lib.spasm_amd_blocks_det(None, out) == -1 and "spasm_amd_blocks_det: NULL handle" in S._abi.last_error()
    assert lib.spasm_amd_dcsr_det(None, out) == -1 and "spasm_amd_dcsr_det: NULL matrix" in S._abi.last_error()
    assert untouched()


def test_count_zero_succeeds_and_clears_the_error(S):
    fn = S._abi.lib().spasm_amd_det_batch
    out, untouched = sentinel_slots(1)
    assert fn(-1, None, out) == -1 and S._abi.last_error() != ""
    assert fn(0, None, None) == 0
    assert S._abi.last_error() == ""
    assert fn(0, csr_array(S, []), out) == 0 and untouched()
    assert S.det_stats() == dict.fromkeys(S.api.DET_STATS, 0)
    d = S.det_batch([])
    assert isinstance(d, np.ndarray) and d.dtype == np.int64 and d.shape == (0,)


def test_python_wrappers_check_their_arguments(S):
    with pytest.raises(TypeError):
        S.det_batch([square(S), np.zeros((2, 2), dtype=np.int64)])
    with pytest.raises(TypeError):
        S.det(np.zeros((2, 2), dtype=np.int64))
    with pytest.raises(S.SpasmError, match=r"not square \(3 x 2\)"):
        S.det(tall(S))
    with pytest.raises(S.SpasmError, match=r"matrix 1: not square \(3 x 2\)"):
        S.det_batch([square(S), tall(S)])
    S._abi.lib().spasm_amd_det_stats(None)  # ignored, not dereferenced


def test_det_fails_loudly_without_gpu(S):
    if S._abi.lib().spasm_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    A, B = square(S), square(S, prime=65521)
    out, untouched = sentinel_slots(2)
    assert S._abi.lib().spasm_amd_det_batch(2, csr_array(S, [A, B]), out) == -1
    assert "no HIP device" in S._abi.last_error()
    assert S._abi.lib().spasm_amd_det(A.data, out) == -1 and "no HIP device" in S._abi.last_error()
    assert untouched()
    with pytest.raises(S.SpasmError, match="no HIP device"):
        S.det_batch([A, B])
    with pytest.raises(S.SpasmError, match="no HIP device"):
        S.det(A)
