"""CPU tests of the dense apply of the resident solver (spasm_amd_solver_apply_dense / _dev / _dense_info): symbols, bindings, the
handle of zero systems, the argument checks of the C entry points -- which come before anything touches a device -- and the
argument checks of BatchSolver.solve_dense, which come before any C call.  Nothing here needs a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

DENSE_SYMBOLS = ["spasm_amd_solver_apply_dense", "spasm_amd_solver_apply_dense_dev", "spasm_amd_solver_dense_info"]
SENTINEL = 0x5A5A5A5A
OKFILL = 0xA5


def windows(rows=4, K=3):
    B = np.full((rows, K), 7, dtype=np.int32)
    X = np.full((rows, K), SENTINEL, dtype=np.int32)
    ok = np.full(rows * K, OKFILL, dtype=np.uint8)
    return B, X, ok, lambda: (B == 7).all() and (X == SENTINEL).all() and (ok == OKFILL).all()


def test_dense_symbols_exported_with_the_documented_signatures(S):
    lib = S._abi.lib()
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    want = {
        "spasm_amd_solver_apply_dense": (i32, [vp, i32, vp, i64, vp, i64, vp]),
        "spasm_amd_solver_apply_dense_dev": (i32, [vp, i32, vp, i64, vp, i64, vp, vp]),
        "spasm_amd_solver_dense_info": (None, [vp, C.POINTER(i64)]),
    }
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spasm_amd.h")).read()
    for name in DENSE_SYMBOLS:
        assert name in S._abi.SIGNATURES, name
        assert S._abi.SIGNATURES[name] == want[name], name
        fn = getattr(lib, name)
        assert fn.restype == want[name][0] and fn.argtypes == want[name][1], name
        assert name + "(" in hdr, name
    assert "int spasm_amd_solver_apply_dense_dev(spasm_amd_solver *S, int K, const spasm_ZZp *B, i64 ldb, spasm_ZZp *X, i64 ldx, unsigned char *ok, void *stream);" in hdr
    assert callable(S.BatchSolver.solve_dense) and callable(S.BatchSolver.dense_info)
    assert len(S.api.SOLVER_DENSE_INFO) == 8 and len(set(S.api.SOLVER_DENSE_INFO)) == 8


def test_a_solver_of_zero_systems_applies_without_a_device_and_writes_nothing(S):
    lib = S._abi.lib()
    h = lib.spasm_amd_solver_create(0, None)
    assert h
    B, X, ok, untouched = windows()
    for fn, tail in ((lib.spasm_amd_solver_apply_dense, ()), (lib.spasm_amd_solver_apply_dense_dev, (None,))):
        assert fn(h, 3, B.ctypes.data, 3, X.ctypes.data, 3, ok.ctypes.data, *tail) == 0 and S._abi.last_error() == ""
        assert fn(h, 0, None, 0, None, 0, None, *tail) == 0 and S._abi.last_error() == ""
        assert fn(h, 3, None, 5, None, 4, None, *tail) == 0
        assert untouched()
    info = (C.c_int64 * 8)(*[7] * 8)
    lib.spasm_amd_solver_dense_info(h, info)
    assert list(info) == [0] * 8
    lib.spasm_amd_solver_dense_info(None, info)   # ignored, not dereferenced
    lib.spasm_amd_solver_dense_info(h, None)
    lib.spasm_amd_solver_free(h)
    with S.BatchSolver([]) as sv:
        assert sv.dense_info() == dict.fromkeys(S.api.SOLVER_DENSE_INFO, 0)
        Xn, okn = sv.solve_dense(np.zeros((0, 3), dtype=np.int32))
        assert Xn.shape == (0, 3) and okn.shape == (0, 3)
    with pytest.raises(S.SpasmError, match="closed"):
        sv.solve_dense(np.zeros((0, 3), dtype=np.int32))


@pytest.mark.parametrize("entry", ["spasm_amd_solver_apply_dense", "spasm_amd_solver_apply_dense_dev"])
def test_argument_errors_return_minus_one_name_the_function_and_leave_the_outputs(S, entry):
    lib = S._abi.lib()
    fn = getattr(lib, entry)
    tail = (None,) if entry.endswith("_dev") else ()
    h = lib.spasm_amd_solver_create(0, None)
    B, X, ok, untouched = windows()

    def failed(rc, word):
        e = S._abi.last_error()
        return rc == -1 and e.startswith(entry + ":") and word in e and untouched()

    assert failed(fn(None, 3, B.ctypes.data, 3, X.ctypes.data, 3, ok.ctypes.data, *tail), "NULL handle")
    assert failed(fn(h, -1, B.ctypes.data, 3, X.ctypes.data, 3, ok.ctypes.data, *tail), "K < 0")
    assert failed(fn(h, 3, B.ctypes.data, 2, X.ctypes.data, 3, ok.ctypes.data, *tail), "ldb < K")
    assert failed(fn(h, 3, B.ctypes.data, 3, X.ctypes.data, 2, ok.ctypes.data, *tail), "ldx < K")
    # the handle stays usable and the error text is empty after success
    assert fn(h, 3, B.ctypes.data, 3, X.ctypes.data, 3, ok.ctypes.data, *tail) == 0 and S._abi.last_error() == "" and untouched()
    lib.spasm_amd_solver_free(h)


def test_python_argument_checks_raise_before_any_c_call(S, monkeypatch):
    """A solver of two empty-shaped systems (0 x 3 and 2 x 0: no device at create) stands for a 2 x 3 matrix."""
    A0 = S.CSR.from_rows([], 3, prime=127)
    Am = S.CSR.from_rows([[], []], 0, prime=127)
    with S.BatchSolver([A0, Am]) as sv:
        info = sv.dense_info()
        assert (info["rows"], info["cols"], info["ok_rows"], info["general_path"], info["plan_k"], info["plans_built"]) == (2, 3, 2, 0, 0, 0)

        class NoCall:
            def __getattr__(self, name):
                raise AssertionError(f"{name} was called")

        monkeypatch.setattr(S._abi, "lib", lambda: NoCall())
        good = np.zeros((3, 4), dtype=np.int32)
        with pytest.raises(TypeError):
            sv.solve_dense(np.zeros((3, 4), dtype=np.int64))            # wrong dtype
        with pytest.raises(TypeError):
            sv.solve_dense([[0] * 4] * 3)                               # not an array
        with pytest.raises(TypeError):
            sv.solve_dense(good, X=np.zeros((2, 4), dtype=np.int64))
        with pytest.raises(ValueError):
            sv.solve_dense(np.zeros((2, 4), dtype=np.int32))            # wrong shape: M = 3
        with pytest.raises(ValueError):
            sv.solve_dense(np.zeros((3, 4, 1), dtype=np.int32))
        with pytest.raises(ValueError):
            sv.solve_dense(good, X=np.zeros((3, 4), dtype=np.int32))    # N = 2
        with pytest.raises(ValueError):
            sv.solve_dense(np.zeros((4, 3), dtype=np.int32).T)          # no unit stride along the rows
        ro = np.zeros((2, 4), dtype=np.int32)
        ro.flags.writeable = False
        with pytest.raises(ValueError, match="writable"):
            sv.solve_dense(good, X=ro)                                  # read-only X
        both = np.zeros((5, 4), dtype=np.int32)
        with pytest.raises(ValueError, match="overlap"):
            sv.solve_dense(both[:3], X=both[2:4])
        monkeypatch.undo()


def test_dense_apply_fails_loudly_without_gpu(S):
    if S._abi.lib().spasm_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    A0 = S.CSR.from_rows([], 3, prime=127)
    with S.BatchSolver([A0]) as sv:
        B, X, ok, untouched = windows(3, 2)
        rc = S._abi.lib().spasm_amd_solver_apply_dense(sv._need(), 2, B.ctypes.data, 2, None, 2, ok.ctypes.data)
        assert rc == -1 and S._abi.last_error().startswith("spasm_amd_solver_apply_dense:") and "no HIP device" in S._abi.last_error() and untouched()
        assert S._abi.lib().spasm_amd_solver_apply_dense(sv._need(), 2, None, 2, None, 2, ok.ctypes.data) == -1 and "NULL array" in S._abi.last_error()
        assert S._abi.lib().spasm_amd_solver_apply_dense(sv._need(), 0, None, 0, None, 0, None) == 0 and S._abi.last_error() == ""
        with pytest.raises(S.SpasmError, match="no HIP device"):
            sv.solve_dense(np.zeros((3, 2), dtype=np.int32))
