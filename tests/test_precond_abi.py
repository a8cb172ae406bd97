"""CPU tests of the preconditioned Wiedemann boundary (spasm_amd_precond_diagonal / _precond_sequence / _wiedemann_rank* /
_wiedemann_det* / _precond_stats): symbols and bindings, the documented generator of the diagonals against its restatement in
Python integers (tests/precond_ref.py), the argument checks that come before anything touches a device, and the empty cases that
need none.  Nothing here needs a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import precond_ref as R
from wiedemann_ref import PRIMES, bal

SENTINEL = 0x5A5A5A5A
SYMBOLS = [
    "spasm_amd_precond_diagonal", "spasm_amd_precond_sequence", "spasm_amd_wiedemann_rank", "spasm_amd_spmv_wiedemann_rank",
    "spasm_amd_dcsr_wiedemann_rank", "spasm_amd_wiedemann_det", "spasm_amd_spmv_wiedemann_det", "spasm_amd_dcsr_wiedemann_det",
    "spasm_amd_precond_stats",
]


def test_precond_symbols_exported_with_the_documented_signatures(S):
    lib = S._abi.lib()
    for name in SYMBOLS:
        assert name in S._abi.SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.restype == S._abi.SIGNATURES[name][0] and fn.argtypes == S._abi.SIGNATURES[name][1], name
    for name in ("wiedemann_rank", "wiedemann_det", "precond_diagonal", "precond_sequence", "precond_stats"):
        assert callable(getattr(S, name)), name
        assert name in S.__all__, name
    for cls in (S.SpMV, S.DeviceCSR):
        assert callable(cls.wiedemann_rank) and callable(cls.wiedemann_det)
    assert len(S.api.PRECOND_STATS) == 10 and len(set(S.api.PRECOND_STATS)) == 10
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spasm_amd.h")).read()
    for decl in (
        "int spasm_amd_precond_diagonal(int len, uint64_t seed, int which, i64 prime, spasm_ZZp *d);",
        "int spasm_amd_wiedemann_rank(const struct spasm_csr *A, int K, uint64_t seed, int tries, int maxdeg, i64 *rank, int *certain);",
        "int spasm_amd_spmv_wiedemann_rank(spasm_amd_spmv *op, int K, uint64_t seed, int tries, int maxdeg, i64 *rank, int *certain);",
        "int spasm_amd_dcsr_wiedemann_rank(const spasm_amd_dcsr *D, int K, uint64_t seed, int tries, int maxdeg, i64 *rank, int *certain);",
        "int spasm_amd_wiedemann_det(const struct spasm_csr *A, int K, uint64_t seed, int tries, spasm_ZZp *det, int *status);",
        "int spasm_amd_spmv_wiedemann_det(spasm_amd_spmv *op, int K, uint64_t seed, int tries, spasm_ZZp *det, int *status);",
        "int spasm_amd_dcsr_wiedemann_det(const spasm_amd_dcsr *D, int K, uint64_t seed, int tries, spasm_ZZp *det, int *status);",
        "void spasm_amd_precond_stats(i64 *out);",
        "lower bound, always",
    ):
        assert decl in hdr, decl


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("p", PRIMES)
def test_precond_diagonal_follows_the_generator_of_the_header(S, p, which):
    length, seed = 37, 0xC0FFEE
    d = S.precond_diagonal(length, seed, which, p)
    want = R.diagonal(length, seed, which, p)
    assert all(1 <= w < p for w in want)
    assert d.dtype == np.int32 and d.tolist() == bal(np.array(want, dtype=object), p).tolist()
    assert not (d == 0).any()                                      # no zero word, p = 3 included
    assert (np.abs(d.astype(np.int64)) <= p // 2).all()            # balanced
    assert S.precond_diagonal(length, seed, which, p).tobytes() == d.tobytes()   # the same seed, the same bytes
    assert p == 3 or S.precond_diagonal(length, seed + 1, which, p).tobytes() != d.tobytes()
    if which == 1:                                                 # E is the square of a word of 1 .. p - 1
        assert all(pow(w, (p - 1) // 2, p) == 1 for w in want)
    assert S.precond_diagonal(0, seed, which, p).size == 0


def test_precond_diagonal_streams_are_disjoint_from_those_of_the_vectors():
    """Pins the ARGUMENT of the header, not the code: the index fields of the two generators as the header states them cannot
    meet.  It calls nothing of the library; that the library follows these formulas is what
    test_precond_diagonal_follows_the_generator_of_the_header and test_minpoly_abi's vector test pin, word for word."""
    # the vectors use the indices 2 * e + t + 1 <= 2 * n * K < 2^32 for n < 2^24, K <= 64; the diagonals start at 2^60 and their
    # fields (which + 1, block < 2^30, round < 4, half word < 2^16) do not overlap
    assert 2 * (2**24 - 1) * 64 < 2**32
    assert (2**31 // 2) << 20 < 2**60 and 3 << 16 < 1 << 20 and 2**16 <= 1 << 16
    seed, p = 5, 65521
    states_uv = {(seed + R.GOLD * k) & R.M64 for k in range(1, 2 * 40 * 8 + 1)}
    states_d = {(seed + R.GOLD * (((w + 1) << 60) + (r << 16) + h)) & R.M64 for w in (0, 1) for r in range(4) for h in range(256)}
    assert len(states_d) == 2 * 4 * 256 and not (states_uv & states_d)


@pytest.mark.parametrize("p", PRIMES)
def test_precond_diagonal_words_differ_while_they_can(S, p):
    """the first p - 1 words of the left diagonal are a permutation of 1 .. p - 1 (all of them for a small prime, a prefix
    without a repeat for a large one), and so is every later block of p - 1"""
    if p < 1000:
        d = S.precond_diagonal(2 * (p - 1) + 1, 99, 0, p).astype(np.int64) % p
        for blk in (d[: p - 1], d[p - 1: 2 * (p - 1)]):
            assert sorted(blk.tolist()) == list(range(1, p))
        assert p == 3 or d[: p - 1].tolist() != d[p - 1: 2 * (p - 1)].tolist()
    else:
        d = S.precond_diagonal(5000, 99, 0, p)
        assert len(set(d.tolist())) == 5000
    assert len(set(S.precond_diagonal(64, 0, 0, 127).tolist())) == 64   # the identity of order 64 over GF(127) is separated


def test_argument_checks_that_fail_before_any_device(S):
    lib = S._abi.lib()
    err = S._abi.last_error
    rank, certain = C.c_int64(-7), C.c_int32(-7)
    det, status = C.c_int32(-7), C.c_int32(-7)
    buf = (C.c_int32 * 8)(*([SENTINEL] * 8))
    untouched = lambda: (rank.value, certain.value, det.value, status.value) == (-7, -7, -7, -7) and list(buf) == [SENTINEL] * 8
    pr, pc, pd, ps = C.byref(rank), C.byref(certain), C.byref(det), C.byref(status)

    # NULL handles
    for name, tail in (("spasm_amd_wiedemann_rank", (8, 0, 3, 0, pr, pc)), ("spasm_amd_dcsr_wiedemann_rank", (8, 0, 3, 0, pr, pc)),
                       ("spasm_amd_wiedemann_det", (8, 0, 3, pd, ps)), ("spasm_amd_dcsr_wiedemann_det", (8, 0, 3, pd, ps))):
        assert getattr(lib, name)(None, *tail) == -1 and err() == f"{name}: NULL matrix"
    for name, tail in (("spasm_amd_spmv_wiedemann_rank", (8, 0, 3, 0, pr, pc)), ("spasm_amd_spmv_wiedemann_det", (8, 0, 3, pd, ps)),
                       ("spasm_amd_precond_sequence", (1, 1, 4, buf, buf, buf, 1, buf, 1, buf))):
        assert getattr(lib, name)(None, *tail) == -1 and err() == f"{name}: NULL operator"
    assert untouched()

    tall = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)], []], 2, prime=127)
    sq = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)]], 2, prime=127)
    # the determinant wants a square matrix
    assert lib.spasm_amd_wiedemann_det(tall.data, 8, 0, 3, pd, ps) == -1 and err() == "spasm_amd_wiedemann_det: not square (3 x 2)"
    with pytest.raises(S.SpasmError, match=r"not square \(3 x 2\)"):
        S.wiedemann_det(tall)
    # K = 65 (and a negative K)
    assert lib.spasm_amd_wiedemann_rank(tall.data, 65, 0, 3, 0, pr, pc) == -1
    assert err() == "spasm_amd_wiedemann_rank: K out of range (0 <= K <= 64, 0 means 8)"
    assert lib.spasm_amd_wiedemann_rank(tall.data, -1, 0, 3, 0, pr, pc) == -1 and "K out of range" in err()
    assert lib.spasm_amd_wiedemann_det(sq.data, 65, 0, 3, pd, ps) == -1 and "K out of range" in err()
    # NULL outputs
    assert lib.spasm_amd_wiedemann_rank(tall.data, 8, 0, 3, 0, None, pc) == -1 and err() == "spasm_amd_wiedemann_rank: NULL array"
    assert lib.spasm_amd_wiedemann_rank(tall.data, 8, 0, 3, 0, pr, None) == -1 and err() == "spasm_amd_wiedemann_rank: NULL array"
    assert lib.spasm_amd_wiedemann_det(sq.data, 8, 0, 3, None, ps) == -1 and err() == "spasm_amd_wiedemann_det: NULL array"
    assert lib.spasm_amd_wiedemann_det(sq.data, 8, 0, 3, pd, None) == -1 and err() == "spasm_amd_wiedemann_det: NULL array"
    # (a CSR cannot carry a prime outside 3 .. 0xFFFFFFFB: the generator below is where that check is reached)
    assert untouched()
    # the wrapper's own checks
    with pytest.raises(TypeError):
        S.wiedemann_rank(np.zeros((2, 2)))
    with pytest.raises(TypeError):
        S.precond_sequence(None, 0, None, None, None, None, 4)

    # the generator
    gen = lib.spasm_amd_precond_diagonal
    assert gen(-1, 0, 0, 127, buf) == -1 and "bad arguments (len >= 0, which 0 or 1)" in err()
    assert gen(4, 0, 2, 127, buf) == -1 and "bad arguments" in err()
    assert gen(4, 0, 0, 2, buf) == -1 and "prime out of range" in err()
    assert gen(4, 0, 0, 4294967296, buf) == -1 and "prime out of range" in err()
    assert gen(4, 0, 0, 127, None) == -1 and err() == "spasm_amd_precond_diagonal: NULL array"
    assert untouched()
    assert gen(0, 0, 0, 127, None) == 0 and err() == ""


def test_the_empty_cases_succeed_without_a_device(S):
    for n, m in ((0, 0), (0, 5), (4, 0)):
        E = S.CSR.from_rows([[] for _ in range(n)], m, prime=65521)
        assert S.wiedemann_rank(E) == (0, True)
        assert S._abi.last_error() == ""
    E = S.CSR.from_rows([], 0, prime=65521)
    assert S.wiedemann_det(E) == (1, 1)
    assert S._abi.last_error() == ""
    assert R.rank(R.Mat.from_dense(np.zeros((4, 0))), 65521)[:2] == (0, True) and R.det(R.Mat.from_dense(np.zeros((0, 0))), 65521)[:2] == (1, 1)


def test_every_call_clears_the_stats(S):
    lib = S._abi.lib()
    zero = {k: 0 for k in S.api.PRECOND_STATS}
    S.precond_diagonal(3, 0, 0, 127)
    assert S.precond_stats() == zero
    rank, certain = C.c_int64(0), C.c_int32(0)
    assert lib.spasm_amd_wiedemann_rank(None, 8, 0, 3, 0, C.byref(rank), C.byref(certain)) == -1
    assert S.precond_stats() == zero
    S.wiedemann_rank(S.CSR.from_rows([[], []], 0, prime=127))
    assert S.precond_stats() == zero
    S.wiedemann_det(S.CSR.from_rows([], 0, prime=127))
    assert S.precond_stats() == zero


def test_the_host_reference_keeps_the_contract_on_small_matrices():
    """precond_ref alone: the bound never exceeds the rank of elimination, reaches it for a large prime, and a status 1
    determinant is the determinant of elimination."""
    rng = np.random.default_rng(2024)
    for p in (3, 127, 65521, 4294967291):
        for _ in range(4):
            n, m, r = int(rng.integers(2, 9)), int(rng.integers(2, 9)), int(rng.integers(0, 3))
            D = (rng.integers(0, p, size=(n, r)).astype(object) @ rng.integers(0, p, size=(r, m)).astype(object)) % p
            true = R.eliminate(D, p)[0]
            got, certain, _ = R.rank(R.Mat.from_dense(np.array(D.tolist(), dtype=np.int64)), p, K=2, tries=1)
            assert got <= true and (p < 65521 or got == true) and (not certain or got == min(n, m))
            Q = rng.integers(0, p, size=(n, n))
            v, status, _ = R.det(R.Mat.from_dense(Q), p, K=2, tries=2)
            assert status == 0 or v % p == R.eliminate(Q, p)[1]
