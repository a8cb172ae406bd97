"""CPU tests of the block Wiedemann boundary (spasm_amd_block_sequence* / _block_berlekamp_massey / _block_wiedemann_det* /
_block_stats): symbols and bindings, the argument checks that come before anything touches a device, the empty case that needs
none, and the Python restatement (tests/block_wiedemann_ref.py) checked on sequences whose generator is known by hand.  Nothing here
needs a GPU.  (A zero word in d_left is refused against an operator's prime, and an operator needs a device:
tests/test_gpu_block_wiedemann.py has that refusal.)"""
import ctypes as C
import os
import random

import numpy as np
import pytest

import block_wiedemann_ref as R

SENTINEL = 0x5A5A5A5A
SYMBOLS = [
    "spasm_amd_block_sequence", "spasm_amd_block_sequence_dev", "spasm_amd_block_berlekamp_massey", "spasm_amd_block_wiedemann_det",
    "spasm_amd_spmv_block_wiedemann_det", "spasm_amd_dcsr_block_wiedemann_det", "spasm_amd_block_stats",
]


def test_block_symbols_exported_with_the_documented_signatures(S):
    lib = S._abi.lib()
    for name in SYMBOLS:
        assert name in S._abi.SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.restype == S._abi.SIGNATURES[name][0] and fn.argtypes == S._abi.SIGNATURES[name][1], name
    for name in ("block_sequence", "block_berlekamp_massey", "block_wiedemann_det", "block_stats"):
        assert callable(getattr(S, name)), name
        assert name in S.__all__, name
    assert callable(S.SpMV.block_sequence) and callable(S.SpMV.block_wiedemann_det) and callable(S.DeviceCSR.block_wiedemann_det)
    assert len(S.api.BLOCK_STATS) == 10 and len(set(S.api.BLOCK_STATS)) == 10
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spasm_amd.h")).read()
    for decl in (
        "int spasm_amd_block_sequence(spasm_amd_spmv *op, int trans, int b, int len, const spasm_ZZp *d_left, const spasm_ZZp *U, i64 ldu,",
        "int spasm_amd_block_sequence_dev(spasm_amd_spmv *op, int trans, int b, int len, const spasm_ZZp *d_left, const spasm_ZZp *U, i64 ldu,",
        "int spasm_amd_block_berlekamp_massey(int b, int len, const spasm_ZZp *S, i64 prime, spasm_ZZp *coef, int *rowdeg, int *dmax);",
        "int spasm_amd_block_wiedemann_det(const struct spasm_csr *A, int b, uint64_t seed, int tries, spasm_ZZp *det, int *status);",
        "int spasm_amd_spmv_block_wiedemann_det(spasm_amd_spmv *op, int b, uint64_t seed, int tries, spasm_ZZp *det, int *status);",
        "int spasm_amd_dcsr_block_wiedemann_det(const spasm_amd_dcsr *D, int b, uint64_t seed, int tries, spasm_ZZp *det, int *status);",
        "void spasm_amd_block_stats(i64 *out);",
        "IS MONTE CARLO",
    ):
        assert decl in hdr, decl
    # the word of the scalar routine is not copied: nothing in the block documentation calls status 1 certain
    start = hdr.index("---- block Wiedemann")
    assert "certain" not in hdr[start:]
    assert "Monte Carlo" in S.block_wiedemann_det.__doc__ and "certain" not in S.block_wiedemann_det.__doc__


def test_argument_checks_that_fail_before_any_device(S):
    lib = S._abi.lib()
    err = S._abi.last_error
    det, status, dmax = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)
    buf = (C.c_int32 * 64)(*([SENTINEL] * 64))
    untouched = lambda: (det.value, status.value, dmax.value) == (-7, -7, -7) and list(buf) == [SENTINEL] * 64
    pd, ps, pm = C.byref(det), C.byref(status), C.byref(dmax)

    # NULL handles
    for name in ("spasm_amd_block_wiedemann_det", "spasm_amd_dcsr_block_wiedemann_det"):
        assert getattr(lib, name)(None, 8, 0, 3, pd, ps) == -1 and err() == f"{name}: NULL matrix"
    assert lib.spasm_amd_spmv_block_wiedemann_det(None, 8, 0, 3, pd, ps) == -1 and err() == "spasm_amd_spmv_block_wiedemann_det: NULL operator"
    assert lib.spasm_amd_block_sequence(None, 0, 2, 4, None, buf, 2, buf, 2, buf) == -1 and err() == "spasm_amd_block_sequence: NULL operator"
    assert lib.spasm_amd_block_sequence_dev(None, 0, 2, 4, None, buf, 2, buf, 2, buf, None) == -1
    assert err() == "spasm_amd_block_sequence_dev: NULL operator"
    assert untouched()

    tall = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)], []], 2, prime=127)
    sq = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)]], 2, prime=127)
    # a square matrix
    assert lib.spasm_amd_block_wiedemann_det(tall.data, 8, 0, 3, pd, ps) == -1 and err() == "spasm_amd_block_wiedemann_det: not square (3 x 2)"
    with pytest.raises(S.SpasmError, match=r"not square \(3 x 2\)"):
        S.block_wiedemann_det(tall)
    # the block widths
    for b in (0, 1, 3, 5, 12, 32, -2):
        assert lib.spasm_amd_block_wiedemann_det(sq.data, b, 0, 3, pd, ps) == -1 and err() == "spasm_amd_block_wiedemann_det: b must be 2, 4, 8 or 16"
        assert lib.spasm_amd_block_berlekamp_massey(b, 4, buf, 127, buf, buf, pm) == -1
        assert err() == "spasm_amd_block_berlekamp_massey: b must be 2, 4, 8 or 16"
    with pytest.raises(S.SpasmError, match="b must be 2, 4, 8 or 16"):
        S.block_wiedemann_det(sq, b=3)
    # NULL outputs
    assert lib.spasm_amd_block_wiedemann_det(sq.data, 8, 0, 3, None, ps) == -1 and err() == "spasm_amd_block_wiedemann_det: NULL array"
    assert lib.spasm_amd_block_wiedemann_det(sq.data, 8, 0, 3, pd, None) == -1 and err() == "spasm_amd_block_wiedemann_det: NULL array"
    assert untouched()

    # Berlekamp-Massey over matrix sequences: len, the prime, NULL arrays
    bm = lib.spasm_amd_block_berlekamp_massey
    for ln in (0, -1, 1 << 24):
        assert bm(2, ln, buf, 127, buf, buf, pm) == -1 and "len out of range (1 <= len < 2^24)" in err()
    for p in (2, 1, 0, -5, 4294967296):
        assert bm(2, 4, buf, p, buf, buf, pm) == -1 and "prime out of range" in err()
    for p in (4, 65536, 4294967290):
        assert bm(2, 4, buf, p, buf, buf, pm) == -1 and err() == "spasm_amd_block_berlekamp_massey: prime must be odd"
    for args in ((None, 127, buf, buf, pm), (buf, 127, None, buf, pm), (buf, 127, buf, None, pm), (buf, 127, buf, buf, None)):
        assert bm(2, 4, *args) == -1 and err() == "spasm_amd_block_berlekamp_massey: NULL array"
    assert untouched()
    # the wrapper's own checks
    with pytest.raises(TypeError):
        S.block_wiedemann_det(np.zeros((2, 2)))
    with pytest.raises(TypeError):
        S.block_sequence(None, None, None, 4)
    with pytest.raises(ValueError):
        S.block_berlekamp_massey(np.zeros((4, 2, 3), dtype=np.int32), 127)
    with pytest.raises(TypeError):
        S.block_berlekamp_massey(np.zeros((4, 2, 2)), 127)


def test_the_empty_matrix_has_determinant_one_without_a_device(S):
    E = S.CSR.from_rows([], 0, prime=65521)
    assert S.block_wiedemann_det(E) == (1, 1)
    assert S._abi.last_error() == ""
    assert S.block_stats() == {k: 0 for k in S.api.BLOCK_STATS}


def test_block_entries_fail_loudly_without_gpu(S):
    if S._abi.lib().spasm_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    sq = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)]], 2, prime=127)
    det, status = C.c_int32(-7), C.c_int32(-7)
    assert S._abi.lib().spasm_amd_block_wiedemann_det(sq.data, 2, 0, 3, C.byref(det), C.byref(status)) == -1
    assert S._abi.last_error().startswith("spasm_amd_block_wiedemann_det") and "no HIP device" in S._abi.last_error()
    assert (det.value, status.value) == (-7, -7)
    with pytest.raises(S.SpasmError, match="no HIP device"):
        S.block_wiedemann_det(sq, b=2)
    with pytest.raises(S.SpasmError, match="no HIP device"):
        S.block_berlekamp_massey(np.zeros((4, 2, 2), dtype=np.int32), 127)


def test_the_reference_finds_x_minus_c_for_powers_of_a_block_companion_matrix():
    """S_i = C^i for a 2 x 2 matrix C has the left generator F = x I - C (up to row operations: the reference's elimination takes the
    rows of S_0 = I as pivots and returns it with leading matrix -I)."""
    p = 101
    Cm = [[3, 5], [7, 11]]
    seq = [[[1, 0], [0, 1]]]
    for _ in range(5):
        seq.append(R.mat_mul(seq[-1], Cm, p))
    F, rowdeg = R.generator(seq, 2, p)
    assert rowdeg == [1, 1] and len(F) == 2
    lead = R.leading_matrix(F, rowdeg)
    assert R.det_mod(lead, p) != 0
    # normalised by the leading matrix: lead^-1 F = x I - C
    inv = [[lead[1][1], -lead[0][1]], [-lead[1][0], lead[0][0]]]
    dinv = pow(R.det_mod(lead, p), p - 2, p)
    inv = [[x * dinv % p for x in r] for r in inv]
    assert R.mat_mul(inv, F[1], p) == [[1, 0], [0, 1]]
    assert R.mat_mul(inv, F[0], p) == [[-x % p for x in r] for r in Cm]
    assert R.check_annihilates(F, rowdeg, seq, p) and R.check_row_reduced(F, rowdeg, p)
    assert R.block_hankel_rank(seq, 2, p) == 2
    # the checkers refuse what is wrong: a generator of too small a degree, and a singular leading matrix
    assert not R.check_annihilates([[[1, 0], [0, 1]]], [0, 0], seq, p)
    assert not R.check_row_reduced([F[0], [[1, 0], [2, 0]]], [1, 1], p)


def test_the_reference_keeps_its_contract_and_the_determinant_on_small_matrices():
    """block_wiedemann_ref alone: (A), (B), the degree sum equal to the rank of the block Hankel matrix, the zero sequence, and a
    status 1 determinant equal to the determinant of elimination"""
    for p in (3, 65521, 4294967291):
        for n, b in ((1, 2), (7, 2), (7, 4), (20, 8), (9, 16)):
            rng = random.Random(1000 * n + b)
            A = [[rng.randrange(p) if rng.random() < 0.4 else 0 for _ in range(n)] for _ in range(n)]
            U = [[rng.randrange(p) for _ in range(b)] for _ in range(n)]
            V = [[rng.randrange(p) for _ in range(b)] for _ in range(n)]
            d = [rng.randrange(1, p) for _ in range(n)]
            length = 2 * -(-n // b) + 2
            seq = R.block_sequence(A, U, V, length, p, d_left=d)
            F, rowdeg = R.generator(seq, b, p)
            assert R.check_annihilates(F, rowdeg, seq, p) and R.check_row_reduced(F, rowdeg, p)
            assert sum(rowdeg) == R.block_hankel_rank(seq, b, p)
            v, st = R.block_det(A, U, V, d, p, length)
            if p > 3:
                assert st == 1
            if st == 1:
                assert v == R.det_mod(A, p), (p, n, b)
    zero = [[[0] * 4 for _ in range(4)] for _ in range(6)]
    F, rowdeg = R.generator(zero, 4, 65521)
    assert rowdeg == [0] * 4 and F == [[[1 if r == c else 0 for c in range(4)] for r in range(4)]]
