"""CPU tests of the device block split's boundary (spasm_amd_blocks_*): symbols, bindings, the argument checks -- which come before
anything touches a device and leave the outputs as they were -- and the untouched host path of Block.from_csr.  Nothing here needs
a GPU."""
import ctypes as C
import os

import numpy as np
import pytest
from test_blocks import make_block_matrix

BLOCKS_SYMBOLS = [
    "spasm_amd_blocks_create", "spasm_amd_blocks_create_dcsr", "spasm_amd_blocks_info", "spasm_amd_blocks_shapes", "spasm_amd_blocks_maps",
    "spasm_amd_blocks_fetch", "spasm_amd_blocks_rank", "spasm_amd_blocks_echelonize", "spasm_amd_blocks_kernel", "spasm_amd_blocks_free",
]
SENTINEL = 0x5A5A5A5A


def small(S, prime=127):
    return S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)], []], 2, prime=prime)


def test_the_ten_symbols_are_exported_and_declared(S):
    lib = S._abi.lib()
    P = C.POINTER
    i32, i64, opts = P(C.c_int32), P(C.c_int64), P(S._abi.EchelonizeOptsStruct)
    want = {
        "spasm_amd_blocks_create": (C.c_void_p, [P(S._abi.CsrStruct)]),
        "spasm_amd_blocks_create_dcsr": (C.c_void_p, [C.c_void_p]),
        "spasm_amd_blocks_info": (None, [C.c_void_p, i64]),
        "spasm_amd_blocks_shapes": (C.c_int32, [C.c_void_p, i32, i32, i64]),
        "spasm_amd_blocks_maps": (C.c_int32, [C.c_void_p, i32, i32, i32, i32, i32, i64, i32, i64]),
        "spasm_amd_blocks_fetch": (P(S._abi.CsrStruct), [C.c_void_p, C.c_int32]),
        "spasm_amd_blocks_rank": (C.c_int32, [C.c_void_p, opts, i64]),
        "spasm_amd_blocks_echelonize": (C.c_int32, [C.c_void_p, opts, P(P(S._abi.LuStruct))]),
        "spasm_amd_blocks_kernel": (C.c_int32, [C.c_void_p, opts, P(P(S._abi.CsrStruct))]),
        "spasm_amd_blocks_free": (None, [C.c_void_p]),
    }
    assert sorted(want) == sorted(BLOCKS_SYMBOLS)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spasm_amd.h")).read()
    for name in BLOCKS_SYMBOLS:
        assert S._abi.SIGNATURES.get(name) == want[name], name
        fn = getattr(lib, name)
        assert fn.restype == want[name][0] and fn.argtypes == want[name][1], name
        assert name + "(" in hdr, name
    assert callable(S.DeviceBlocks) and len(S.api.BLOCKS_INFO) == 11


def test_create_refuses_bad_arguments_with_a_text(S):
    lib = S._abi.lib()

    def refused(ptr, *words):
        assert not lib.spasm_amd_blocks_create(ptr)
        err = S._abi.last_error()
        assert err.startswith("spasm_amd_blocks_create: ") and all(w in err for w in words), err

    refused(None, "NULL")
    # no values
    A = small(S)
    refused(S.submatrix(A, range(0, 3), range(0, 2), with_values=False).data, "x == NULL")
    # a prime outside the batch's range
    for p in (2, 0xFFFFFFFB + 6):
        B = small(S)
        B.data.contents.field.p = p
        refused(B.data, "prime out of range")
        B.data.contents.field.p = 127
    # decreasing row pointers
    B = small(S)
    B.p[1], B.p[2] = 3, 2
    refused(B.data, "row pointers must not decrease")
    B.p[1], B.p[2] = 2, 3
    B.p[0] = 1
    refused(B.data, "malformed")
    B.p[0] = 0
    # n + m >= 2^31: refused before the row pointers are read
    B.data.contents.n, B.data.contents.m = 1 << 30, 1 << 30
    refused(B.data, "2^31")
    B.data.contents.n, B.data.contents.m = 3, 2
    assert not lib.spasm_amd_blocks_create_dcsr(None)
    assert "spasm_amd_blocks_create_dcsr" in S._abi.last_error() and "NULL" in S._abi.last_error()


def test_a_null_handle_is_refused_and_the_outputs_stay(S):
    lib = S._abi.lib()
    i32 = lambda: np.full(4, SENTINEL, dtype=np.int32)
    i64 = lambda: np.full(4, SENTINEL, dtype=np.int64)
    p32, p64 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)))

    def failed(rc, name):
        assert rc == -1
        assert name in S._abi.last_error() and "NULL" in S._abi.last_error(), S._abi.last_error()

    info = i64()
    lib.spasm_amd_blocks_info(None, p64(info))  # void: ignored, not dereferenced
    assert (info == SENTINEL).all()
    a, b, c = i32(), i32(), i64()
    failed(lib.spasm_amd_blocks_shapes(None, p32(a), p32(b), p64(c)), "spasm_amd_blocks_shapes")
    assert (a == SENTINEL).all() and (b == SENTINEL).all() and (c == SENTINEL).all()
    m = [i32(), i32(), i32(), i32(), i32(), i64(), i32(), i64()]
    args = [p64(x) if x.dtype == np.int64 else p32(x) for x in m]
    failed(lib.spasm_amd_blocks_maps(None, *args), "spasm_amd_blocks_maps")
    assert all((x == SENTINEL).all() for x in m)
    assert not lib.spasm_amd_blocks_fetch(None, 0)
    assert "spasm_amd_blocks_fetch" in S._abi.last_error() and "NULL" in S._abi.last_error()
    r = i64()
    failed(lib.spasm_amd_blocks_rank(None, None, p64(r)), "spasm_amd_blocks_rank")
    assert (r == SENTINEL).all()
    lus = (C.POINTER(S._abi.LuStruct) * 2)()
    ks = (C.POINTER(S._abi.CsrStruct) * 2)()
    for out in (lus, ks):
        raw = C.cast(out, C.POINTER(C.c_uint64))
        raw[0] = raw[1] = SENTINEL
    failed(lib.spasm_amd_blocks_echelonize(None, None, lus), "spasm_amd_blocks_echelonize")
    failed(lib.spasm_amd_blocks_kernel(None, None, ks), "spasm_amd_blocks_kernel")
    for out in (lus, ks):
        raw = C.cast(out, C.POINTER(C.c_uint64))
        assert raw[0] == SENTINEL and raw[1] == SENTINEL
    lib.spasm_amd_blocks_free(None)  # a no-op


def test_python_wrapper_checks_its_arguments(S):
    with pytest.raises(TypeError):
        S.DeviceBlocks(np.zeros((2, 2), dtype=np.int64))
    if S._abi.lib().spasm_amd_device_count() == 0:
        with pytest.raises(S.SpasmError, match="no HIP device"):
            S.DeviceBlocks(small(S))
        with pytest.raises(S.SpasmError, match="no HIP device"):
            S.Block.from_csr(small(S), device=True)


def test_owner_with_device_blocks_is_a_value_error(S):
    D = object.__new__(S.DeviceBlocks)  # no handle: the check comes before any use of it
    D._h = None
    for fn in (S.blocks.rank, S.blocks.echelonize, S.blocks.kernel):
        with pytest.raises(ValueError, match="owner"):
            fn(D, owner=(0, 2))


def test_from_csr_without_the_keyword_is_the_host_split(S):
    A, nblocks = make_block_matrix(S)
    B = S.Block.from_csr(A)
    assert len(B) == nblocks + 2 and B.shape == A.shape
    assert sorted(i for rows in B.block2row for i in rows) == list(range(A.n))
    assert sorted(c for cols in B.block2col for c in cols) == list(range(A.m))
    for b, blk in enumerate(B.blocks):
        assert blk.shape == (len(B.block2row[b]), len(B.block2col[b]))
        assert B.block2row[b] == sorted(B.block2row[b]) and B.block2col[b] == sorted(B.block2col[b])
    firsts = [min(r + [A.n + c for c in cs]) for r, cs in zip(B.block2row, B.block2col)]
    assert firsts == sorted(firsts)  # numbered by their smallest vertex, rows before columns
    assert B.to_csr().rows() == A.rows()
    B2 = S.Block.from_csr(A, device=False)
    assert (B2.row2block, B2.col2block, B2.block2row, B2.block2col) == (B.row2block, B.col2block, B.block2row, B.block2col)
