"""CPU tests of the solve boundary (spasm_amd_solve_batch / _blocks_solve / _solve_stats): symbols, bindings, the argument checks
-- which come before anything touches a device and leave the output slots as they were -- and the loud failure without a GPU.
Nothing here needs one."""
import ctypes as C
import os

import numpy as np
import pytest

SOLVE_SYMBOLS = ["spasm_amd_solve_batch", "spasm_amd_blocks_solve", "spasm_amd_solve_stats"]
SENTINEL = 0x5A5A5A5A
OKFILL = 0xA5


def small(S, prime=127):
    return S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)], []], 2, prime=prime)


def rhs(S, prime=127, m=2):
    return S.CSR.from_rows([[(0, 1)], [], [(1, 5), (0, 2)]], m, prime=prime)


def csr_array(S, mats):
    return (C.POINTER(S._abi.CsrStruct) * max(len(mats), 1))(*[A.data if A is not None else None for A in mats])


def slots(S, count, rows=3):
    """X slots and ok bytes filled with recognisable patterns, and a function that tells whether they still hold them"""
    out = (C.POINTER(S._abi.CsrStruct) * count)()
    raw = C.cast(out, C.POINTER(C.c_uint64))
    for i in range(count):
        raw[i] = SENTINEL
    oks = [np.full(rows, OKFILL, dtype=np.uint8) for _ in range(count)]
    okp = (C.POINTER(C.c_ubyte) * count)(*[o.ctypes.data_as(C.POINTER(C.c_ubyte)) for o in oks])
    return out, okp, lambda: all(raw[i] == SENTINEL for i in range(count)) and all((o == OKFILL).all() for o in oks)


def test_solve_symbols_exported_with_the_documented_signatures(S):
    lib = S._abi.lib()
    P = C.POINTER
    csrpp = P(P(S._abi.CsrStruct))
    want = {
        "spasm_amd_solve_batch": (C.c_int32, [C.c_int32, csrpp, csrpp, csrpp, P(P(C.c_ubyte))]),
        "spasm_amd_blocks_solve": (C.c_int32, [C.c_void_p, P(S._abi.CsrStruct), csrpp, P(C.c_ubyte)]),
        "spasm_amd_solve_stats": (None, [P(C.c_int64)]),
    }
    for name in SOLVE_SYMBOLS:
        assert name in S._abi.SIGNATURES, name
        assert S._abi.SIGNATURES[name] == want[name], name
        fn = getattr(lib, name)
        assert fn.restype == want[name][0] and fn.argtypes == want[name][1], name
    for name in ("solve_batch", "solve_stats"):
        assert callable(getattr(S, name)), name
    assert callable(S.DeviceBlocks.solve) and callable(S.blocks.solve)
    assert len(S.api.SOLVE_STATS) == 8 and len(set(S.api.SOLVE_STATS)) == 8
    assert len(S.api.BATCH_STATS) == 8 and len(S.api.BLOCKS_INFO) == 11
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spasm_amd.h")).read()
    for name in SOLVE_SYMBOLS:
        assert name + "(" in hdr, name
    # the contract: the canonical basis on the LDS path, its absence on the general path, the equality of the two routes
    assert "CANONICAL ROW BASIS" in hdr and "DOES NOT HOLD" in hdr and "BYTE FOR BYTE" in hdr


def test_argument_errors_return_minus_one_and_leave_the_slots(S):
    fn = S._abi.lib().spasm_amd_solve_batch
    err = S._abi.last_error
    A, B = small(S), rhs(S)
    out, okp, untouched = slots(S, 3)
    assert fn(-1, csr_array(S, [A]), csr_array(S, [B]), out, okp) == -1
    assert "count < 0" in err() and err().startswith("spasm_amd_solve_batch")
    # a NULL array: of matrices, of right-hand sides, of outputs, of ok
    for args in ((None, csr_array(S, [B, B]), out, okp), (csr_array(S, [A, A]), None, out, okp), (csr_array(S, [A, A]), csr_array(S, [B, B]), None, okp),
                 (csr_array(S, [A, A]), csr_array(S, [B, B]), out, None)):
        assert fn(2, *args) == -1 and "NULL array" in err()
    # a NULL matrix on either side: the index is named
    assert fn(3, csr_array(S, [A, None, A]), csr_array(S, [B, B, B]), out, okp) == -1
    assert "matrix 1" in err() and "NULL matrix" in err()
    assert fn(3, csr_array(S, [A, A, A]), csr_array(S, [B, B, None]), out, okp) == -1
    assert "matrix 2" in err() and "NULL matrix" in err()
    # a matrix without values
    Pat = S.submatrix(A, range(0, 3), range(0, 2), with_values=False)
    assert fn(3, csr_array(S, [A, A, Pat]), csr_array(S, [B, B, B]), out, okp) == -1
    assert "matrix 2" in err() and "x == NULL" in err()
    BPat = S.submatrix(B, range(0, 3), range(0, 2), with_values=False)
    assert fn(2, csr_array(S, [A, A]), csr_array(S, [BPat, B]), out, okp) == -1
    assert "matrix 0" in err() and "x == NULL" in err()
    # primes that differ, column counts that differ
    assert fn(2, csr_array(S, [A, A]), csr_array(S, [B, rhs(S, prime=65521)]), out, okp) == -1
    assert "matrix 1" in err() and "primes" in err()
    assert fn(2, csr_array(S, [A, A]), csr_array(S, [rhs(S, m=3), B]), out, okp) == -1
    assert "matrix 0" in err() and "B->m != A->m" in err()
    # a column index outside the matrix, in A and in B
    A2 = small(S)
    A2.j[2] = 2
    assert fn(2, csr_array(S, [A, A2]), csr_array(S, [B, B]), out, okp) == -1
    assert "matrix 1" in err() and "column index" in err()
    B2 = rhs(S)
    B2.j[0] = -1
    assert fn(2, csr_array(S, [A, A]), csr_array(S, [B, B2]), out, okp) == -1
    assert "matrix 1" in err() and "column index" in err()
    # malformed row pointers
    A3 = small(S)
    A3.p[2] = 1
    assert fn(1, csr_array(S, [A3]), csr_array(S, [B]), out, okp) == -1
    assert "matrix 0" in err() and "row pointers" in err()
    assert untouched()


def test_blocks_solve_argument_errors_without_a_handle(S):
    fn = S._abi.lib().spasm_amd_blocks_solve
    out, okp, untouched = slots(S, 1)
    assert fn(None, rhs(S).data, out, okp[0]) == -1
    assert S._abi.last_error().startswith("spasm_amd_blocks_solve") and "NULL handle" in S._abi.last_error()
    assert untouched()


def test_count_zero_succeeds_clears_the_error_and_zeroes_the_stats(S):
    fn = S._abi.lib().spasm_amd_solve_batch
    out, okp, untouched = slots(S, 1)
    assert fn(-1, None, None, out, okp) == -1 and S._abi.last_error() != ""
    assert fn(0, None, None, None, None) == 0
    assert S._abi.last_error() == ""
    assert fn(0, csr_array(S, []), csr_array(S, []), out, okp) == 0 and untouched()
    assert S.solve_stats() == dict.fromkeys(S.api.SOLVE_STATS, 0)
    assert S.solve_batch([], []) == ([], [])
    S._abi.lib().spasm_amd_solve_stats(None)  # ignored, not dereferenced


def test_systems_of_empty_shape_need_no_device(S):
    """n = 0: only the zero row is reachable; m = 0: everything is; K = 0: nothing to do"""
    p = 127
    A0 = S.CSR.from_rows([], 3, prime=p)                      # 0 x 3
    B0 = S.CSR.from_arrays(3, 3, [0, 1, 3, 3], [2, 0, 1], [5, 0, p], prime=p)   # a non-zero row, a row of stored zeros, an empty row
    Am = S.CSR.from_rows([[], []], 0, prime=p)                # 2 x 0
    Bm = S.CSR.from_rows([[], [], []], 0, prime=p)
    Ak = small(S)
    Bk = S.CSR.from_rows([], 2, prime=p)                      # K = 0
    X, ok = S.solve_batch([A0, Am, Ak], [B0, Bm, Bk])
    assert [x.shape for x in X] == [(3, 0), (3, 2), (0, 3)] and all(S.nnz(x) == 0 for x in X)
    assert ok[0].tolist() == [False, True, True] and ok[1].tolist() == [True, True, True] and ok[2].tolist() == []
    assert all(o.dtype == np.bool_ for o in ok)
    st = S.solve_stats()
    assert (st["systems"], st["lds_path"], st["general_path"], st["jobs"], st["launches"], st["unsolved"]) == (3, 3, 0, 0, 0, 1)


def test_python_wrappers_check_their_arguments(S, monkeypatch):
    with pytest.raises(TypeError):
        S.solve_batch([small(S), np.zeros((2, 2), dtype=np.int64)], [rhs(S), rhs(S)])
    with pytest.raises(TypeError):
        S.solve_batch([small(S)], [[1, 2]])
    with pytest.raises(ValueError):
        S.solve_batch([small(S), small(S)], [rhs(S)])
    A = small(S)
    Bk = S.Block([A], [(0, 0), (0, 1), (0, 2)], [(0, 0), (0, 1)], [[0, 1, 2]], [[0, 1]])
    with pytest.raises(TypeError):
        S.blocks.solve(Bk, np.zeros((1, 2)))
    with pytest.raises(ValueError):
        S.blocks.solve(Bk, rhs(S, m=3))
    # the host Block route deals the columns of B to the blocks and goes through ONE solve_batch call
    calls = []

    def fake(mats, rs):
        calls.append((len(mats), [r.rows() for r in rs]))
        return [S.CSR.from_rows([[(1, 4)], [(0, 2), (2, 3)]], 3, prime=127)], [np.array([True, False])]

    monkeypatch.setattr(S.api, "solve_batch", fake)
    X, ok = S.blocks.solve(Bk, rhs(S))
    assert calls == [(1, [[[(0, 1)], [(0, 2), (1, 5)]]])]   # the empty row of B reaches no block
    assert ok.tolist() == [True, True, False] and X.rows() == [[(1, 4)], [], []] and X.shape == (3, 3)


def test_solve_fails_loudly_without_gpu(S):
    if S._abi.lib().spasm_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    A, B = small(S), rhs(S)
    out, okp, untouched = slots(S, 2)
    assert S._abi.lib().spasm_amd_solve_batch(2, csr_array(S, [A, A]), csr_array(S, [B, B]), out, okp) == -1
    assert "no HIP device" in S._abi.last_error()
    assert untouched()
    with pytest.raises(S.SpasmError, match="no HIP device"):
        S.solve_batch([A], [B])
    with pytest.raises(S.SpasmError, match="no HIP device"):
        S.DeviceBlocks(A)
