"""CPU tests of the batch boundary (spasm_amd_echelonize_batch / _rank_batch / _kernel_batch / _batch_stats): symbols, bindings,
the argument checks -- which come before anything touches a device and leave the output slots as they were -- and the loud failure
without a GPU.  Nothing here needs one."""
import ctypes as C

import numpy as np
import pytest

BATCH_SYMBOLS = ["spasm_amd_echelonize_batch", "spasm_amd_rank_batch", "spasm_amd_kernel_batch", "spasm_amd_batch_stats"]
SENTINEL = 0x5A5A5A5A


def small(S, prime=127):
    return S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)], []], 2, prime=prime)


def csr_array(S, mats):
    return (C.POINTER(S._abi.CsrStruct) * max(len(mats), 1))(*[A.data if A is not None else None for A in mats])


def sentinel_slots(S, kind, count):
    """output slots filled with a recognisable pattern, and a function that tells whether they still hold it"""
    if kind == "rank":
        out = (C.c_int64 * count)(*([SENTINEL] * count))
        return out, lambda: all(out[i] == SENTINEL for i in range(count))
    struct = S._abi.LuStruct if kind == "echelonize" else S._abi.CsrStruct
    out = (C.POINTER(struct) * count)()
    raw = C.cast(out, C.POINTER(C.c_uint64))
    for i in range(count):
        raw[i] = SENTINEL
    return out, lambda: all(raw[i] == SENTINEL for i in range(count))


def entry(S, kind):
    return getattr(S._abi.lib(), f"spasm_amd_{kind}_batch")


def test_batch_symbols_exported_with_the_documented_signatures(S):
    lib = S._abi.lib()
    P = C.POINTER
    csrpp, opts = P(P(S._abi.CsrStruct)), P(S._abi.EchelonizeOptsStruct)
    want = {
        "spasm_amd_echelonize_batch": (C.c_int32, [C.c_int32, csrpp, opts, P(P(S._abi.LuStruct))]),
        "spasm_amd_rank_batch": (C.c_int32, [C.c_int32, csrpp, opts, P(C.c_int64)]),
        "spasm_amd_kernel_batch": (C.c_int32, [C.c_int32, csrpp, opts, P(P(S._abi.CsrStruct))]),
        "spasm_amd_batch_stats": (None, [P(C.c_int64)]),
    }
    for name in BATCH_SYMBOLS:
        assert name in S._abi.SIGNATURES, name
        assert S._abi.SIGNATURES[name] == want[name], name
        fn = getattr(lib, name)
        assert fn.restype == want[name][0] and fn.argtypes == want[name][1], name
    for name in ("echelonize_batch", "rank_batch", "kernel_batch", "batch_stats"):
        assert callable(getattr(S, name)), name
    assert len(S.api.BATCH_STATS) == 8
    # the header declares them, with the note that the pivot-search options have no effect on the LDS path
    import os

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spasm_amd.h")).read()
    for name in BATCH_SYMBOLS:
        assert name + "(" in hdr, name
    assert "NO EFFECT" in hdr


@pytest.mark.parametrize("kind", ["echelonize", "rank", "kernel"])
def test_argument_errors_return_minus_one_and_leave_the_slots(S, kind):
    fn = entry(S, kind)
    A = small(S)
    out, untouched = sentinel_slots(S, kind, 3)
    # count < 0
    assert fn(-1, csr_array(S, [A]), None, out) == -1
    assert "count < 0" in S._abi.last_error() and f"spasm_amd_{kind}_batch" in S._abi.last_error()
    # a NULL array (of matrices, of outputs)
    assert fn(2, None, None, out) == -1 and "NULL array" in S._abi.last_error()
    assert fn(2, csr_array(S, [A, A]), None, None) == -1 and "NULL array" in S._abi.last_error()
    # a NULL matrix: the index is named
    assert fn(3, csr_array(S, [A, None, A]), None, out) == -1
    assert "matrix 1" in S._abi.last_error() and "NULL matrix" in S._abi.last_error()
    # a matrix without values
    Pat = S.submatrix(A, range(0, 3), range(0, 2), with_values=False)
    assert fn(3, csr_array(S, [A, A, Pat]), None, out) == -1
    assert "matrix 2" in S._abi.last_error() and "x == NULL" in S._abi.last_error()
    # a column index outside the matrix
    B = small(S)
    B.j[2] = 2
    assert fn(2, csr_array(S, [A, B]), None, out) == -1
    assert "matrix 1" in S._abi.last_error() and "column index" in S._abi.last_error()
    B.j[2] = -1
    assert fn(2, csr_array(S, [A, B]), None, out) == -1 and "column index" in S._abi.last_error()
    assert untouched()


@pytest.mark.parametrize("kind", ["echelonize", "rank", "kernel"])
def test_count_zero_succeeds_and_clears_the_error(S, kind):
    fn = entry(S, kind)
    out, untouched = sentinel_slots(S, kind, 1)
    assert fn(-1, None, None, out) == -1 and S._abi.last_error() != ""
    assert fn(0, None, None, None) == 0
    assert S._abi.last_error() == ""
    assert fn(0, csr_array(S, []), None, out) == 0 and untouched()
    assert S.batch_stats() == dict.fromkeys(S.api.BATCH_STATS, 0)
    assert {"echelonize": S.echelonize_batch, "rank": S.rank_batch, "kernel": S.kernel_batch}[kind]([]) == []


def test_python_wrappers_check_their_arguments(S):
    with pytest.raises(TypeError):
        S.echelonize_batch([small(S), np.zeros((2, 2), dtype=np.int64)])
    with pytest.raises(AttributeError):
        S.rank_batch([small(S)], no_such_option=1)
    S._abi.lib().spasm_amd_batch_stats(None)  # ignored, not dereferenced


def test_blocks_keep_the_loop_by_default(S, monkeypatch):
    """batched=False (the default) never reaches a batch entry; batched=True sends the caller's share through one call"""
    calls = []
    monkeypatch.setattr(S.api, "echelonize", lambda A, **kw: calls.append(("one", kw)) or "lu")
    monkeypatch.setattr(S.api, "echelonize_batch", lambda mats, **kw: calls.append(("batch", len(mats), kw)) or ["lu"] * len(mats))
    monkeypatch.setattr(S.api, "rank_batch", lambda mats, **kw: calls.append(("rank_batch", len(mats), kw)) or [1] * len(mats))
    blocks = [small(S) for _ in range(5)]
    B = S.Block(blocks, [], [], [[] for _ in blocks], [[] for _ in blocks])
    E = S.blocks.echelonize(B, enable_dense=False)
    assert calls == [("one", {"enable_dense": False})] * 5 and E.blocks == ["lu"] * 5
    calls.clear()
    E = S.blocks.echelonize(B, owner=(1, 2), batched=True, enable_dense=False)
    assert calls == [("batch", 2, {"enable_dense": False})]
    assert E.blocks == [None, "lu", None, "lu", None]
    calls.clear()
    assert S.blocks.rank(B, owner=(0, 2), batched=True) == 3 and calls == [("rank_batch", 3, {})]


@pytest.mark.parametrize("kind", ["echelonize", "rank", "kernel"])
def test_batch_fails_loudly_without_gpu(S, kind):
    if S._abi.lib().spasm_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    A, B = small(S), small(S, prime=65521)
    out, untouched = sentinel_slots(S, kind, 2)
    assert entry(S, kind)(2, csr_array(S, [A, B]), None, out) == -1
    assert "no HIP device" in S._abi.last_error()
    assert untouched()
    with pytest.raises(S.SpasmError, match="no HIP device"):
        {"echelonize": S.echelonize_batch, "rank": S.rank_batch, "kernel": S.kernel_batch}[kind]([A, B])
