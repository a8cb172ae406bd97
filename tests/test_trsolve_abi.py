"""CPU tests of the dense triangular solves' boundary (spasm_dense_forward_solve, spasm_dense_back_solve, spasm_amd_trsolve_*):
symbols, bindings and the argument checks that happen in Python before any C call.  Nothing here needs a GPU."""
import numpy as np
import pytest

TRSOLVE_SYMBOLS = ["spasm_dense_forward_solve", "spasm_dense_back_solve", "spasm_amd_trsolve_create", "spasm_amd_trsolve_apply",
                   "spasm_amd_trsolve_apply_dev", "spasm_amd_trsolve_free"]


def small(S):
    # 2 x 3: [[1, 2, 0], [0, 1, 5]]
    return S.CSR.from_arrays(2, 3, np.array([0, 2, 4]), np.array([0, 1, 1, 2], dtype=np.int32), np.array([1, 2, 1, 5], dtype=np.int32),
                             prime=42013)


def test_trsolve_symbols_exported_and_bound(S):
    lib = S._abi.lib()
    for name in TRSOLVE_SYMBOLS + ["spasm_amd_trsolve_stats"]:
        assert name in S._abi.SIGNATURES, name
        assert getattr(lib, name).argtypes == S._abi.SIGNATURES[name][1], name
    assert callable(S.dense_forward_solve) and callable(S.dense_back_solve) and S.TriangularSolver is not None
    assert S._abi.SIGNATURES["spasm_dense_forward_solve"][0] is S._abi.C.c_bool


def i32(*shape):
    return np.zeros(shape, dtype=np.int32)


@pytest.mark.parametrize(
    "call",
    [
        lambda S, T: S.dense_forward_solve(T, i32(2), i32(2), i32(2)),        # b has T.m = 3 entries
        lambda S, T: S.dense_forward_solve(T, i32(3), i32(3), i32(2)),        # x has T.n = 2 entries
        lambda S, T: S.dense_forward_solve(T, i32(3), i32(2), i32(3)),        # q has T.n = 2 entries
        lambda S, T: S.dense_back_solve(T, i32(3), i32(2), i32(2)),           # p has T.m = 3 entries
        lambda S, T: S.dense_back_solve(T, i32(2), i32(2), i32(3)),
        lambda S, T: S.dense_back_solve(T, i32(3), i32(3), i32(3)),
        lambda S, T: S.dense_forward_solve(T, i32(3, 1), i32(2), i32(2)),
        lambda S, T: S.TriangularSolver(T, i32(3), "forward"),
        lambda S, T: S.TriangularSolver(T, i32(2), "back"),
        lambda S, T: S.TriangularSolver(T, i32(2), "sideways"),
    ],
)
def test_wrong_lengths_rejected_in_python(S, call, monkeypatch):
    T = small(S)
    monkeypatch.setattr(S._abi, "lib", lambda: pytest.fail("a C call was made"))
    with pytest.raises(ValueError):
        call(S, T)


@pytest.mark.parametrize(
    "call",
    [
        lambda S, T: S.dense_forward_solve(T, np.zeros(3, np.int64), i32(2), i32(2)),
        lambda S, T: S.dense_forward_solve(T, i32(3), np.zeros(2, np.float32), i32(2)),
        lambda S, T: S.dense_forward_solve(T, i32(3), i32(2), np.zeros(2, np.int64)),
        lambda S, T: S.dense_back_solve(T, [0, 0, 0], i32(2), i32(3)),
        lambda S, T: S.dense_back_solve(T, i32(3), np.zeros(2, np.uint32), i32(3)),
        lambda S, T: S.TriangularSolver(T, [0, 1], "forward"),
        lambda S, T: S.TriangularSolver(T, np.zeros(3, np.int64), "back"),
    ],
)
def test_wrong_dtypes_rejected_in_python(S, call, monkeypatch):
    T = small(S)
    monkeypatch.setattr(S._abi, "lib", lambda: pytest.fail("a C call was made"))
    with pytest.raises(TypeError):
        call(S, T)


def test_readonly_arrays_rejected_in_python(S, monkeypatch):
    T = small(S)
    monkeypatch.setattr(S._abi, "lib", lambda: pytest.fail("a C call was made"))
    b = i32(3)
    b.flags.writeable = False
    with pytest.raises(ValueError):
        S.dense_forward_solve(T, b, i32(2), i32(2))


def test_solves_fail_loudly_without_gpu(S):
    if S._abi.lib().spasm_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    T = small(S)
    b = np.array([7, -8, 9], dtype=np.int32)
    x = np.array([1, 2], dtype=np.int32)
    with pytest.raises(S.SpasmError, match="no HIP device"):
        S.dense_forward_solve(T, b, x, np.array([0, 1], dtype=np.int32))
    with pytest.raises(S.SpasmError, match="no HIP device"):
        S.dense_back_solve(T, b, x, np.array([0, 1, -1], dtype=np.int32))
    assert b.tolist() == [7, -8, 9] and x.tolist() == [1, 2]
    with pytest.raises(S.SpasmError, match="no HIP device"):
        S.TriangularSolver(T, np.array([0, 1], dtype=np.int32))


def test_null_arguments_are_errors_not_faults(S):
    lib = S._abi.lib()
    assert not lib.spasm_amd_trsolve_create(None, None, 0)
    assert S._abi.last_error()
    assert lib.spasm_amd_trsolve_apply(None, 1, None, 1, None, 1, None) == -1
    assert "NULL operator" in S._abi.last_error()
    assert not lib.spasm_dense_forward_solve(None, None, None, None)
    assert S._abi.last_error().startswith("spasm_dense_forward_solve")
    lib.spasm_amd_trsolve_free(None)
