"""CPU tests of the exact products' boundary (spasm_Axpy, spasm_xApy, spasm_amd_spmv_*): symbols, bindings and the argument checks
that happen in Python before any C call.  Nothing here needs a GPU."""
import numpy as np
import pytest

SPMV_SYMBOLS = ["spasm_Axpy", "spasm_xApy", "spasm_amd_spmv_create", "spasm_amd_spmv_apply", "spasm_amd_spmv_apply_dev", "spasm_amd_spmv_free"]


def small(S):
    return S.CSR(np.array([[1, 2, 0], [3, 6, 5]]))  # stored transpose: 3 x 2


def test_spmv_symbols_exported_and_bound(S):
    lib = S._abi.lib()
    for name in SPMV_SYMBOLS:
        assert name in S._abi.SIGNATURES, name
        assert getattr(lib, name).argtypes == S._abi.SIGNATURES[name][1], name
    assert callable(S.axpy) and callable(S.xapy) and S.SpMV is not None


@pytest.mark.parametrize(
    "call",
    [
        lambda S, A: S.axpy(A, np.zeros(3, np.int32), np.zeros(3, np.int32)),   # x has A.m = 2 entries
        lambda S, A: S.axpy(A, np.zeros(2, np.int32), np.zeros(2, np.int32)),   # y has A.n = 3 entries
        lambda S, A: S.xapy(np.zeros(2, np.int32), A, np.zeros(2, np.int32)),   # x has A.n = 3 entries
        lambda S, A: S.xapy(np.zeros(3, np.int32), A, np.zeros(3, np.int32)),   # y has A.m = 2 entries
        lambda S, A: A @ np.zeros(3, np.int64),
        lambda S, A: np.zeros(2, np.int64) @ A,
        lambda S, A: A @ np.zeros((3, 4), np.int64),
        lambda S, A: np.zeros((4, 2), np.int64) @ A,
        lambda S, A: A @ np.zeros((2, 2, 2), np.int64),
    ],
)
def test_wrong_lengths_rejected_in_python(S, call):
    with pytest.raises(ValueError):
        call(S, small(S))


@pytest.mark.parametrize(
    "call",
    [
        lambda S, A: S.axpy(A, np.zeros(2, np.int64), np.zeros(3, np.int32)),
        lambda S, A: S.axpy(A, np.zeros(2, np.int32), np.zeros(3, np.float32)),
        lambda S, A: S.xapy([0, 0, 0], A, np.zeros(2, np.int32)),
        lambda S, A: S.xapy(np.zeros(3, np.int32), A, np.zeros(2, np.uint32)),
        lambda S, A: A @ np.zeros(2, np.float64),
    ],
)
def test_wrong_dtypes_rejected_in_python(S, call):
    with pytest.raises(TypeError):
        call(S, small(S))


def test_ndarray_matmul_reaches_rmatmul(S, monkeypatch):
    """`ndarray @ CSR` must reach CSR.__rmatmul__, not numpy's own matmul"""
    seen = []
    monkeypatch.setattr(S.api, "_product", lambda A, x, trans: seen.append(trans) or "ok")
    A = small(S)
    assert np.arange(3) @ A == "ok" and A @ np.arange(2) == "ok"
    assert seen == [True, False]


def test_products_fail_loudly_without_gpu(S):
    if S._abi.lib().spasm_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    A = small(S)
    y = np.array([7, -8, 9], dtype=np.int32)
    with pytest.raises(S.SpasmError, match="no HIP device"):
        S.axpy(A, np.array([1, 2], dtype=np.int32), y)
    assert y.tolist() == [7, -8, 9]
    y2 = np.array([5, 6], dtype=np.int32)
    with pytest.raises(S.SpasmError, match="no HIP device"):
        S.xapy(np.array([1, 2, 3], dtype=np.int32), A, y2)
    assert y2.tolist() == [5, 6]
    with pytest.raises(S.SpasmError, match="no HIP device"):
        S.SpMV(A)
    with pytest.raises(S.SpasmError, match="no HIP device"):
        A @ np.array([3, -1])
