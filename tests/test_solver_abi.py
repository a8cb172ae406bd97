"""CPU tests of the resident solver's boundary (spasm_amd_solver_*): symbols, bindings, the argument checks of create -- which come
before anything touches a device -- the handle of zero systems, which never needs one, and the loud failure without a GPU.  Nothing
here needs one."""
import ctypes as C
import os

import numpy as np
import pytest

SOLVER_SYMBOLS = ["spasm_amd_solver_create", "spasm_amd_solver_create_blocks", "spasm_amd_solver_apply", "spasm_amd_solver_apply_blocks", "spasm_amd_solver_info",
                  "spasm_amd_solver_ranks", "spasm_amd_solver_basis", "spasm_amd_solver_stats", "spasm_amd_solver_free"]
SENTINEL = 0x5A5A5A5A
OKFILL = 0xA5


def small(S, prime=127):
    return S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)], []], 2, prime=prime)


def rhs(S, prime=127, m=2):
    return S.CSR.from_rows([[(0, 1)], [], [(1, 5), (0, 2)]], m, prime=prime)


def csr_array(S, mats):
    return (C.POINTER(S._abi.CsrStruct) * max(len(mats), 1))(*[A.data if A is not None else None for A in mats])


def slots(S, count, rows=3):
    out = (C.POINTER(S._abi.CsrStruct) * count)()
    raw = C.cast(out, C.POINTER(C.c_uint64))
    for i in range(count):
        raw[i] = SENTINEL
    oks = [np.full(rows, OKFILL, dtype=np.uint8) for _ in range(count)]
    okp = (C.POINTER(C.c_ubyte) * count)(*[o.ctypes.data_as(C.POINTER(C.c_ubyte)) for o in oks])
    return out, okp, lambda: all(raw[i] == SENTINEL for i in range(count)) and all((o == OKFILL).all() for o in oks)


def test_solver_symbols_exported_with_the_documented_signatures(S):
    lib = S._abi.lib()
    P = C.POINTER
    csrp = P(S._abi.CsrStruct)
    csrpp = P(csrp)
    want = {
        "spasm_amd_solver_create": (C.c_void_p, [C.c_int32, csrpp]),
        "spasm_amd_solver_create_blocks": (C.c_void_p, [C.c_void_p]),
        "spasm_amd_solver_apply": (C.c_int32, [C.c_void_p, csrpp, csrpp, P(P(C.c_ubyte))]),
        "spasm_amd_solver_apply_blocks": (C.c_int32, [C.c_void_p, csrp, csrpp, P(C.c_ubyte)]),
        "spasm_amd_solver_info": (None, [C.c_void_p, P(C.c_int64)]),
        "spasm_amd_solver_ranks": (C.c_int32, [C.c_void_p, P(C.c_int64)]),
        "spasm_amd_solver_basis": (C.c_int32, [C.c_void_p, C.c_int32, P(C.c_int32)]),
        "spasm_amd_solver_stats": (None, [P(C.c_int64)]),
        "spasm_amd_solver_free": (None, [C.c_void_p]),
    }
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spasm_amd.h")).read()
    assert "typedef struct spasm_amd_solver spasm_amd_solver;" in hdr   # the tenth name of the interface: the handle's type
    for name in SOLVER_SYMBOLS:
        assert name in S._abi.SIGNATURES, name
        assert S._abi.SIGNATURES[name] == want[name], name
        fn = getattr(lib, name)
        assert fn.restype == want[name][0] and fn.argtypes == want[name][1], name
        assert name + "(" in hdr, name
    assert callable(S.BatchSolver) and callable(S.BatchSolver.from_blocks) and callable(S.DeviceBlocks.solver) and callable(S.solver_stats)
    for name in ("solve", "basis", "info", "close", "__enter__", "__exit__", "__del__"):
        assert callable(getattr(S.BatchSolver, name)), name
    assert isinstance(S.BatchSolver.ranks, property)
    assert len(S.api.SOLVER_INFO) == 8 and len(set(S.api.SOLVER_INFO)) == 8


def test_a_solver_of_zero_systems_needs_no_device(S):
    lib = S._abi.lib()
    h = lib.spasm_amd_solver_create(0, None)
    assert h and S._abi.last_error() == ""
    out, okp, untouched = slots(S, 1)
    assert lib.spasm_amd_solver_apply(h, None, None, None) == 0 and S._abi.last_error() == ""
    assert lib.spasm_amd_solver_apply(h, csr_array(S, []), out, okp) == 0 and untouched()
    info = (C.c_int64 * 8)(*[7] * 8)
    lib.spasm_amd_solver_info(h, info)
    assert list(info) == [0] * 8
    assert lib.spasm_amd_solver_ranks(h, None) == 0
    assert lib.spasm_amd_solver_basis(h, 0, None) == -1 and "spasm_amd_solver_basis" in S._abi.last_error() and "index" in S._abi.last_error()
    # the handle of a list is not one of blocks
    assert lib.spasm_amd_solver_apply_blocks(h, rhs(S).data, out, okp[0]) == -1
    assert S._abi.last_error().startswith("spasm_amd_solver_apply_blocks") and "spasm_amd_solver_create" in S._abi.last_error() and untouched()
    lib.spasm_amd_solver_free(h)
    with S.BatchSolver([]) as sv:
        assert sv.solve([]) == ([], []) and sv.ranks == [] and len(sv) == 0
        assert sv.info() == dict.fromkeys(S.api.SOLVER_INFO, 0)
        assert S.solver_stats() == dict.fromkeys(S.api.SOLVE_STATS, 0)
    with pytest.raises(S.SpasmError, match="closed"):
        sv.solve([])
    lib.spasm_amd_solver_stats(None)  # ignored, not dereferenced
    lib.spasm_amd_solver_info(None, info)


def test_create_argument_errors_return_null_and_name_the_function(S):
    fn = S._abi.lib().spasm_amd_solver_create
    err = S._abi.last_error
    A = small(S)

    def failed(*words):
        e = err()
        return e.startswith("spasm_amd_solver_create:") and all(w in e for w in words)

    assert not fn(-1, csr_array(S, [A])) and failed("count < 0")
    assert not fn(2, None) and failed("NULL array")
    assert not fn(3, csr_array(S, [A, None, A])) and failed("matrix 1", "NULL matrix")
    Pat = S.submatrix(A, range(0, 3), range(0, 2), with_values=False)
    assert not fn(3, csr_array(S, [A, A, Pat])) and failed("matrix 2", "x == NULL")
    A3 = small(S)
    A3.p[2] = 1
    assert not fn(1, csr_array(S, [A3])) and failed("matrix 0", "row pointers")
    A2 = small(S)
    A2.j[2] = 2
    assert not fn(2, csr_array(S, [A, A2])) and failed("matrix 1", "column index")
    assert not S._abi.lib().spasm_amd_solver_create_blocks(None)
    assert err().startswith("spasm_amd_solver_create_blocks") and "NULL handle" in err()


def test_calls_on_a_null_handle_fail_and_leave_the_slots(S):
    lib = S._abi.lib()
    out, okp, untouched = slots(S, 1)
    B = rhs(S)
    assert lib.spasm_amd_solver_apply(None, csr_array(S, [B]), out, okp) == -1
    assert S._abi.last_error().startswith("spasm_amd_solver_apply:") and "NULL handle" in S._abi.last_error()
    assert lib.spasm_amd_solver_apply_blocks(None, B.data, out, okp[0]) == -1
    assert S._abi.last_error().startswith("spasm_amd_solver_apply_blocks:") and "NULL handle" in S._abi.last_error()
    rank = (C.c_int64 * 1)(SENTINEL)
    assert lib.spasm_amd_solver_ranks(None, rank) == -1 and rank[0] == SENTINEL and "spasm_amd_solver_ranks" in S._abi.last_error()
    rows = (C.c_int32 * 1)(77)
    assert lib.spasm_amd_solver_basis(None, 0, rows) == -1 and rows[0] == 77
    assert untouched()
    lib.spasm_amd_solver_free(None)  # harmless


def test_systems_of_empty_shape_need_no_device(S):
    """n = 0: only the zero row is reachable; m = 0: everything is.  Neither is factored, neither is launched."""
    p = 127
    A0 = S.CSR.from_rows([], 3, prime=p)                      # 0 x 3
    B0 = S.CSR.from_arrays(3, 3, [0, 1, 3, 3], [2, 0, 1], [5, 0, p], prime=p)   # a non-zero row, a row of stored zeros, an empty row
    Am = S.CSR.from_rows([[], []], 0, prime=p)                # 2 x 0
    Bm = S.CSR.from_rows([[], [], []], 0, prime=p)
    with S.BatchSolver([A0, Am]) as sv:
        assert sv.ranks == [0, 0] and sv.basis(0).tolist() == [] and sv.basis(1).tolist() == []
        i = sv.info()
        assert (i["systems"], i["lds_path"], i["general_path"], i["operator_words"], i["factor_jobs"], i["create_launches"]) == (2, 2, 0, 0, 0, 0)
        for _ in range(2):
            X, ok = sv.solve([B0, Bm])
            assert [x.shape for x in X] == [(3, 0), (3, 2)] and all(S.nnz(x) == 0 for x in X)
            assert ok[0].tolist() == [False, True, True] and ok[1].tolist() == [True, True, True]
        st = S.solver_stats()
        assert (st["systems"], st["lds_path"], st["general_path"], st["jobs"], st["launches"], st["unsolved"]) == (2, 2, 0, 0, 0, 1)
        # a live handle: the wrong m, the wrong prime, the wrong kind of apply; the outputs stay, the handle stays usable
        out, okp, untouched = slots(S, 2)
        fn = S._abi.lib().spasm_amd_solver_apply
        assert fn(sv._need(), csr_array(S, [B0, S.CSR.from_rows([[]], 1, prime=p)]), out, okp) == -1
        assert "matrix 1" in S._abi.last_error() and "B->m != A->m" in S._abi.last_error()
        assert fn(sv._need(), csr_array(S, [S.CSR.from_rows([[]], 3, prime=65521), Bm]), out, okp) == -1
        assert "matrix 0" in S._abi.last_error() and "primes" in S._abi.last_error()
        assert fn(sv._need(), csr_array(S, [B0, None]), out, okp) == -1 and "matrix 1" in S._abi.last_error()
        assert untouched()
        assert sv.solve([B0, Bm])[1][0].tolist() == [False, True, True]
        with pytest.raises(IndexError):
            sv.basis(2)
        with pytest.raises(ValueError):
            sv.solve([B0])
        with pytest.raises(TypeError):
            sv.solve([B0, np.zeros((1, 1))])
    with pytest.raises(TypeError):
        S.BatchSolver([A0, [1]])
    with pytest.raises(TypeError):
        S.BatchSolver.from_blocks(A0)
    with pytest.raises(TypeError):
        S.blocks.solver(A0)


def test_solver_fails_loudly_without_gpu(S):
    if S._abi.lib().spasm_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    A = small(S)
    assert not S._abi.lib().spasm_amd_solver_create(1, csr_array(S, [A]))
    assert S._abi.last_error().startswith("spasm_amd_solver_create") and "no HIP device" in S._abi.last_error()
    with pytest.raises(S.SpasmError, match="no HIP device"):
        S.BatchSolver([A])
