"""CPU tests of the characteristic polynomial by components: the index split (spasm_amd_blocks_create_index / _create_index_dcsr /
_is_index), the product of polynomials (spasm_amd_poly_product) and the consumers (spasm_amd_blocks_charpoly / _charpoly_factors /
_charpoly_split / _dcsr_charpoly_split / _charpoly_split_stats): symbols, bindings, the argument checks -- which come before
anything touches a device and leave the output as it was -- the loud failure without a GPU, and the host Block.from_csr(A,
index=True), the independent reference of the device maps.  Nothing here needs a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

SENTINEL = 0x5A5A5A5A
I32P = C.POINTER(C.c_int32)


def square(S, prime=127):
    return S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)]], 2, prime=prime)


def tall(S, prime=127):
    return S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)], []], 2, prime=prime)


def cycle3(S, prime=127):
    """the permutation matrix of the 3-cycle: chi = x^3 - 1, and no row shares a column with another"""
    return S.CSR.from_rows([[(1, 1)], [(2, 1)], [(0, 1)]], 3, prime=prime)


def sentinel(words):
    buf = (C.c_int32 * words)(*([SENTINEL] * words))
    return buf, C.cast(buf, I32P), lambda: all(buf[i] == SENTINEL for i in range(words))


def poly_args(polys):
    arrs = [(C.c_int32 * max(len(f), 1))(*f) for f in polys]
    lens = (C.c_int32 * max(len(polys), 1))(*[len(f) for f in polys])
    ptrs = (I32P * max(len(polys), 1))(*[C.cast(a, I32P) for a in arrs])
    return arrs, lens, ptrs


def test_symbols_exported_bound_and_declared(S):
    lib = S._abi.lib()
    P = C.POINTER
    want = {
        "spasm_amd_blocks_create_index": (C.c_void_p, [P(S._abi.CsrStruct)]),
        "spasm_amd_blocks_create_index_dcsr": (C.c_void_p, [C.c_void_p]),
        "spasm_amd_blocks_is_index": (C.c_int32, [C.c_void_p]),
        "spasm_amd_poly_product": (C.c_int32, [C.c_int32, P(C.c_int32), P(P(C.c_int32)), C.c_int64, P(C.c_int32)]),
        "spasm_amd_blocks_charpoly": (C.c_int32, [C.c_void_p, P(C.c_int32)]),
        "spasm_amd_blocks_charpoly_factors": (C.c_int32, [C.c_void_p, P(C.c_int32)]),
        "spasm_amd_charpoly_split": (C.c_int32, [P(S._abi.CsrStruct), P(C.c_int32)]),
        "spasm_amd_dcsr_charpoly_split": (C.c_int32, [C.c_void_p, P(C.c_int32)]),
        "spasm_amd_charpoly_split_stats": (None, [P(C.c_int64)]),
    }
    for name, sig in want.items():
        assert S._abi.SIGNATURES.get(name) == sig, name
        fn = getattr(lib, name)
        assert fn.restype == sig[0] and fn.argtypes == sig[1], name
    for name in ("poly_product", "charpoly_split_stats"):
        assert callable(getattr(S, name)), name
        assert name in S.__all__, name
    assert callable(S.DeviceBlocks.charpoly) and callable(S.DeviceBlocks.charpoly_factors)
    assert isinstance(S.DeviceBlocks.index, property)
    assert callable(S.blocks.charpoly)
    assert len(S.api.CHARPOLY_SPLIT_STATS) == 8 and len(set(S.api.CHARPOLY_SPLIT_STATS)) == 8
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spasm_amd.h")).read()
    for decl in (
        "spasm_amd_blocks *spasm_amd_blocks_create_index(const struct spasm_csr *A);",
        "spasm_amd_blocks *spasm_amd_blocks_create_index_dcsr(const spasm_amd_dcsr *D);",
        "int spasm_amd_blocks_is_index(const spasm_amd_blocks *B);",
        "int spasm_amd_poly_product(int count, const int *len, const spasm_ZZp *const *f, i64 prime, spasm_ZZp *out);",
        "int spasm_amd_blocks_charpoly(spasm_amd_blocks *B, spasm_ZZp *coef);",
        "int spasm_amd_blocks_charpoly_factors(spasm_amd_blocks *B, spasm_ZZp *coef);",
        "int spasm_amd_charpoly_split(const struct spasm_csr *A, spasm_ZZp *coef);",
        "int spasm_amd_dcsr_charpoly_split(const spasm_amd_dcsr *D, spasm_ZZp *coef);",
        "void spasm_amd_charpoly_split_stats(i64 *out);",
    ):
        assert decl in hdr, decl


def test_index_creators_refuse_before_a_device_is_looked_for(S):
    lib = S._abi.lib()
    assert lib.spasm_amd_blocks_is_index(None) == -1
    assert not lib.spasm_amd_blocks_create_index(None)
    assert "spasm_amd_blocks_create_index: NULL matrix" in S._abi.last_error()
    assert not lib.spasm_amd_blocks_create_index_dcsr(None)
    assert "spasm_amd_blocks_create_index_dcsr: NULL matrix" in S._abi.last_error()
    assert not lib.spasm_amd_blocks_create_index(tall(S).data)
    assert "spasm_amd_blocks_create_index: not square (3 x 2)" in S._abi.last_error()
    B = square(S)
    B.data.contents.field.p = 2
    assert not lib.spasm_amd_blocks_create_index(B.data) and "prime out of range" in S._abi.last_error()
    with pytest.raises(S.SpasmError, match=r"not square \(3 x 2\)"):
        S.DeviceBlocks(tall(S), index=True)


def test_poly_product_argument_errors_leave_the_output(S):
    fn = S._abi.lib().spasm_amd_poly_product
    buf, out, untouched = sentinel(8)
    keep, lens, ptrs = poly_args([[1, 2], [3, 4, 5]])
    assert fn(-1, lens, ptrs, 127, out) == -1
    assert "spasm_amd_poly_product: count < 0" in S._abi.last_error()
    assert fn(2, None, ptrs, 127, out) == -1 and "NULL array" in S._abi.last_error()
    assert fn(2, lens, None, 127, out) == -1 and "NULL array" in S._abi.last_error()
    assert fn(2, lens, ptrs, 127, None) == -1 and "NULL array" in S._abi.last_error()
    holed = (I32P * 2)(ptrs[0], None)
    assert fn(2, lens, holed, 127, out) == -1
    assert "polynomial 1" in S._abi.last_error() and "NULL array" in S._abi.last_error()
    zero = (C.c_int32 * 2)(2, 0)
    assert fn(2, zero, ptrs, 127, out) == -1
    assert "polynomial 1" in S._abi.last_error() and "length" in S._abi.last_error()
    for bad in (2, 1, 0, -7, 0xFFFFFFFB + 2):
        assert fn(2, lens, ptrs, bad, out) == -1 and "prime out of range" in S._abi.last_error()
    # a total length of 2^31: the lengths are looked at before any word of a polynomial is
    huge = (C.c_int32 * 2)(2**30, 2**30)
    assert fn(2, huge, ptrs, 127, out) == -1
    assert "polynomial 1" in S._abi.last_error() and "below 2^31" in S._abi.last_error()
    assert untouched()


def test_poly_product_of_nothing_is_one_without_a_device(S):
    fn = S._abi.lib().spasm_amd_poly_product
    buf, out, _ = sentinel(2)
    assert fn(-1, None, None, 127, out) == -1 and S._abi.last_error() != ""
    assert fn(0, None, None, 127, out) == 0
    assert S._abi.last_error() == ""
    assert buf[0] == 1 and buf[1] == SENTINEL
    assert S.poly_product([], 65521).tolist() == [1]
    with pytest.raises(S.SpasmError, match="polynomial 0"):
        S.poly_product([[]], 127)


def test_charpoly_consumers_refuse_null_arguments(S):
    lib = S._abi.lib()
    buf, out, untouched = sentinel(4)
    assert lib.spasm_amd_blocks_charpoly(None, out) == -1 and "spasm_amd_blocks_charpoly: NULL handle" in S._abi.last_error()
    assert lib.spasm_amd_blocks_charpoly_factors(None, out) == -1 and "spasm_amd_blocks_charpoly_factors: NULL handle" in S._abi.last_error()
    assert lib.spasm_amd_charpoly_split(None, out) == -1 and "spasm_amd_charpoly_split: NULL matrix" in S._abi.last_error()
    assert lib.spasm_amd_charpoly_split(square(S).data, None) == -1 and "NULL array" in S._abi.last_error()
    assert lib.spasm_amd_charpoly_split(tall(S).data, out) == -1
    assert "spasm_amd_charpoly_split: not square (3 x 2)" in S._abi.last_error()
    assert lib.spasm_amd_dcsr_charpoly_split(None, out) == -1 and "spasm_amd_dcsr_charpoly_split: NULL matrix" in S._abi.last_error()
    B = square(S)
    B.data.contents.field.p = 2
    assert lib.spasm_amd_charpoly_split(B.data, out) == -1 and "prime out of range" in S._abi.last_error()
    assert untouched()
    lib.spasm_amd_charpoly_split_stats(None)  # ignored, not dereferenced
    with pytest.raises(TypeError):
        S.charpoly(np.zeros((2, 2), dtype=np.int64), split=True)
    with pytest.raises(S.SpasmError, match=r"not square \(3 x 2\)"):
        S.charpoly(tall(S), split=True)


def test_new_entries_fail_loudly_without_gpu(S):
    if S._abi.lib().spasm_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    lib = S._abi.lib()
    buf, out, untouched = sentinel(8)
    assert not lib.spasm_amd_blocks_create_index(cycle3(S).data) and "no HIP device" in S._abi.last_error()
    assert lib.spasm_amd_charpoly_split(cycle3(S).data, out) == -1 and "no HIP device" in S._abi.last_error()
    keep, lens, ptrs = poly_args([[1, 2], [3, 4, 5]])
    assert lib.spasm_amd_poly_product(2, lens, ptrs, 127, out) == -1 and "no HIP device" in S._abi.last_error()
    assert untouched()
    with pytest.raises(S.SpasmError, match="no HIP device"):
        S.poly_product([[1, 2], [3, 4]], 127)
    with pytest.raises(S.SpasmError, match="no HIP device"):
        S.charpoly(cycle3(S), split=True)
    with pytest.raises(S.SpasmError, match="no HIP device"):
        S.DeviceBlocks(cycle3(S), index=True)


# ---------------------------------------------------------------------------------------------
# the host Block.from_csr(A, index=True)
# ---------------------------------------------------------------------------------------------
def test_three_cycle_is_one_block_by_index_and_three_without(S):
    A = cycle3(S)
    free = S.Block.from_csr(A)
    assert len(free) == 3 and all(X.shape == (1, 1) for X in free.blocks) and not free.index
    B = S.Block.from_csr(A, index=True)
    assert B.index and len(B) == 1 and B.blocks[0].shape == (3, 3)
    assert B.row2block == B.col2block == [(0, 0), (0, 1), (0, 2)]
    assert B.block2row == B.block2col == [[0, 1, 2]]
    assert B.blocks[0].rows() == A.rows()


def test_index_maps_agree_on_random_sparse_matrices(S):
    rng = np.random.default_rng(23)
    for n, per_row in ((1, 1), (7, 1), (40, 1), (200, 1), (200, 2)):
        rows = []
        for i in range(n):
            k = int(rng.integers(0, per_row + 1))
            rows.append([(int(c), int(rng.integers(1, 100))) for c in sorted(set(rng.integers(0, n, size=k).tolist()))])
        A = S.CSR.from_rows(rows, n, prime=127)
        B = S.Block.from_csr(A, index=True)
        assert B.row2block == B.col2block
        assert B.block2row == B.block2col
        assert all(X.n == X.m for X in B.blocks)
        assert [r[0] for r in B.block2row] == sorted(r[0] for r in B.block2row)   # blocks ascend by smallest index
        assert B.to_csr().rows() == A.rows()
        # the components against a plain search over the symmetric index graph
        adj = [set() for _ in range(n)]
        for i, r in enumerate(rows):
            for c, _ in r:
                adj[i].add(c)
                adj[c].add(i)
        seen, comps = [False] * n, []
        for i in range(n):
            if not seen[i]:
                comp, todo = [], [i]
                seen[i] = True
                while todo:
                    v = todo.pop()
                    comp.append(v)
                    for w in adj[v]:
                        if not seen[w]:
                            seen[w] = True
                            todo.append(w)
                comps.append(sorted(comp))
        assert B.block2row == comps


def test_stored_zero_joins_and_bare_index_is_a_zero_block(S):
    # (0, 1) is a stored zero: indices 0 and 1 are one block; index 2 has neither row nor column entries; 3 holds its diagonal
    A = S.CSR.from_rows([[(1, 0)], [(1, 5)], [], [(3, 7)]], 4, prime=127)
    B = S.Block.from_csr(A, index=True)
    assert B.block2row == B.block2col == [[0, 1], [2], [3]]
    assert [X.shape for X in B.blocks] == [(2, 2), (1, 1), (1, 1)]
    assert S.nnz(B.blocks[1]) == 0
    assert B.blocks[0].rows() == [[(1, 0)], [(1, 5)]]


def test_not_square_is_refused_by_the_host_split(S):
    with pytest.raises(ValueError, match=r"not square \(3 x 2\)"):
        S.Block.from_csr(tall(S), index=True)
    with pytest.raises(ValueError, match="not an index split"):
        S.blocks.charpoly(S.Block.from_csr(cycle3(S)))
