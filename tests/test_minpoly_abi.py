"""CPU tests of the Wiedemann boundary (spasm_amd_krylov_sequence / _berlekamp_massey / _poly_lcm / _minpoly* / _minpoly_stats):
symbols and bindings, spasm_amd_poly_lcm (host arithmetic, no device) against Euclid in Python integers, the seeded vectors, and the
argument checks that come before anything touches a device.  Nothing here needs a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

PRIMES = (3, 127, 65521, 2**31 - 1, 4294967291)
SENTINEL = 0x5A5A5A5A
SYMBOLS = [
    "spasm_amd_krylov_sequence", "spasm_amd_krylov_sequence_dev", "spasm_amd_berlekamp_massey", "spasm_amd_poly_lcm",
    "spasm_amd_minpoly_vectors", "spasm_amd_minpoly", "spasm_amd_spmv_minpoly", "spasm_amd_dcsr_minpoly", "spasm_amd_minpoly_stats",
]


# ---------------------------------------------------------------------------------------------
# polynomials over GF(p) in Python integers: lists of residues in [0, p), low degree first, no zero leading word
# ---------------------------------------------------------------------------------------------
def trim(a):
    a = list(a)
    while a and a[-1] == 0:
        a.pop()
    return a


def pmul(a, b, p):
    if not a or not b:
        return []
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % p
    return trim(out)


def pdivmod(a, b, p):
    a, q = list(a), [0] * max(len(a) - len(b) + 1, 0)
    ib = pow(b[-1], -1, p)
    while len(a) >= len(b):
        sh, f = len(a) - len(b), a[-1] * ib % p
        q[sh] = f
        for k, y in enumerate(b):
            a[sh + k] = (a[sh + k] - f * y) % p
        a = trim(a)
    return trim(q), a


def pmonic(a, p):
    i = pow(a[-1], -1, p)
    return [x * i % p for x in a]


def pgcd(a, b, p):
    while b:
        a, b = b, pdivmod(a, b, p)[1]
    return pmonic(a, p)


def plcm(polys, p):
    r = [1]
    for f in polys:
        f = trim([int(x) % p for x in f])
        r = pmonic(pdivmod(pmul(r, f, p), pgcd(r, f, p), p)[0], p)
    return r


def bal(v, p):
    return np.array([x - p if x > p // 2 else x for x in (int(y) % p for y in v)], dtype=np.int32)


def rand_poly(rng, deg, p, monic=True):
    f = [int(rng.integers(0, p)) for _ in range(deg)] + [1 if monic else int(rng.integers(1, p))]
    return f


# ---------------------------------------------------------------------------------------------
def test_minpoly_symbols_exported_with_the_documented_signatures(S):
    lib = S._abi.lib()
    for name in SYMBOLS:
        assert name in S._abi.SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.restype == S._abi.SIGNATURES[name][0] and fn.argtypes == S._abi.SIGNATURES[name][1], name
    for name in ("krylov_sequence", "berlekamp_massey", "poly_lcm", "minpoly", "minpoly_vectors", "minpoly_stats"):
        assert callable(getattr(S, name)), name
        assert name in S.__all__, name
    assert callable(S.SpMV.minpoly) and callable(S.SpMV.krylov_sequence) and callable(S.DeviceCSR.minpoly)
    assert len(S.api.MINPOLY_STATS) == 8 and len(set(S.api.MINPOLY_STATS)) == 8
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spasm_amd.h")).read()
    for decl in (
        "int spasm_amd_krylov_sequence(spasm_amd_spmv *op, int trans, int K, int len, const spasm_ZZp *U, i64 ldu, const spasm_ZZp *V, i64 ldv, spasm_ZZp *S);",
        "int spasm_amd_berlekamp_massey(int count, int len, const spasm_ZZp *S, i64 lds, i64 prime, int where, spasm_ZZp *coef, i64 ldc, int *deg);",
        "int spasm_amd_poly_lcm(int count, const int *len, const spasm_ZZp *const *f, i64 prime, spasm_ZZp *out, int *outlen);",
        "int spasm_amd_minpoly(const struct spasm_csr *A, int K, uint64_t seed, int maxdeg, const spasm_ZZp *U, const spasm_ZZp *V, spasm_ZZp *coef, int *deg);",
        "int spasm_amd_spmv_minpoly(spasm_amd_spmv *op, int K, uint64_t seed, int maxdeg, const spasm_ZZp *U, const spasm_ZZp *V, spasm_ZZp *coef, int *deg);",
        "int spasm_amd_dcsr_minpoly(const spasm_amd_dcsr *D, int K, uint64_t seed, int maxdeg, const spasm_ZZp *U, const spasm_ZZp *V, spasm_ZZp *coef, int *deg);",
        "void spasm_amd_minpoly_stats(i64 *out);",
    ):
        assert decl in hdr, decl


@pytest.mark.parametrize("p", PRIMES)
def test_poly_lcm_matches_euclid_in_python_integers(S, p):
    rng = np.random.default_rng(p % 1000003)
    while True:   # two coprime factors
        f1, f2 = rand_poly(rng, 3, p), rand_poly(rng, 4, p)
        if pgcd(f1, f2, p) == [1]:
            break
    g = rand_poly(rng, 2, p)
    cases = {
        "coprime": [f1, f2],
        "one divides the other": [f1, pmul(f1, g, p)],
        "the other way round": [pmul(f1, g, p), f1],
        "equal": [f2, f2, f2],
        "a constant 1": [[1], f1, [1]],
        "a common factor": [pmul(f1, g, p), pmul(f2, g, p)],
        "not monic, a zero leading word": [rand_poly(rng, 5, p, monic=False) + [0, 0], [int(rng.integers(2, p))]],
        "a long and a short one": [rand_poly(rng, 40, p), pmul(g, g, p), rand_poly(rng, 1, p)],
    }
    for name, polys in cases.items():
        want = plcm(polys, p)
        got = S.poly_lcm([bal(f, p) for f in polys], p)
        assert got.dtype == np.int32 and got[-1] == 1, name
        assert got.tolist() == bal(want, p).tolist(), (name, p)
    # entries need not be reduced: any int32 is taken mod p
    if p < 2**30:
        raw = [np.array([int(x) + p for x in f1], dtype=np.int32), bal(f2, p)]
        assert S.poly_lcm(raw, p).tolist() == bal(plcm([f1, f2], p), p).tolist()
    assert S.poly_lcm([], p).tolist() == [1]


def test_poly_lcm_writes_outlen_words_and_no_more(S):
    lib = S._abi.lib()
    p = 127
    f = [np.array([1, 1], dtype=np.int32), np.array([1, 1], dtype=np.int32)]   # lcm = x + 1: 2 of the 3 words a product would take
    lens = (C.c_int32 * 2)(2, 2)
    ptrs = (C.POINTER(C.c_int32) * 2)(*[a.ctypes.data_as(C.POINTER(C.c_int32)) for a in f])
    out = (C.c_int32 * 4)(*([SENTINEL] * 4))
    outlen = C.c_int32(-7)
    assert lib.spasm_amd_poly_lcm(2, lens, ptrs, p, out, C.byref(outlen)) == 0, S._abi.last_error()
    assert outlen.value == 2 and list(out) == [1, 1, SENTINEL, SENTINEL]
    assert S._abi.last_error() == ""


def test_poly_lcm_argument_errors(S):
    lib = S._abi.lib()
    f = [np.array([1, 1], dtype=np.int32), np.array([0, 0], dtype=np.int32)]
    lens = (C.c_int32 * 2)(2, 2)
    ptrs = (C.POINTER(C.c_int32) * 2)(*[a.ctypes.data_as(C.POINTER(C.c_int32)) for a in f])
    out = (C.c_int32 * 4)(*([SENTINEL] * 4))
    outlen = C.c_int32(-7)
    fn = lib.spasm_amd_poly_lcm
    assert fn(2, lens, ptrs, 127, out, C.byref(outlen)) == -1
    assert S._abi.last_error() == "spasm_amd_poly_lcm: polynomial 1: the zero polynomial has no lcm"
    assert fn(-1, lens, ptrs, 127, out, C.byref(outlen)) == -1 and "count < 0" in S._abi.last_error()
    assert fn(1, lens, ptrs, 2, out, C.byref(outlen)) == -1 and "prime out of range" in S._abi.last_error()
    assert fn(1, lens, ptrs, 127, None, C.byref(outlen)) == -1 and "NULL array" in S._abi.last_error()
    assert fn(1, None, ptrs, 127, out, C.byref(outlen)) == -1 and "NULL array" in S._abi.last_error()
    lens0 = (C.c_int32 * 2)(0, 2)
    assert fn(1, lens0, ptrs, 127, out, C.byref(outlen)) == -1 and "polynomial 0: a length below 1 (0)" in S._abi.last_error()
    assert list(out) == [SENTINEL] * 4 and outlen.value == -7


def splitmix(z):
    M = (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


@pytest.mark.parametrize("p", PRIMES)
def test_minpoly_vectors_follow_the_generator_of_the_header(S, p):
    n, K, seed = 5, 3, 0xC0FFEE
    U, V = S.minpoly_vectors(n, K, seed, p)
    for t, W in ((0, U), (1, V)):
        want = [splitmix((seed + 0x9E3779B97F4A7C15 * (2 * e + t + 1)) & ((1 << 64) - 1)) % p for e in range(n * K)]
        assert W.reshape(-1).tolist() == bal(want, p).tolist()
    U2, V2 = S.minpoly_vectors(n, K, seed, p)
    assert U2.tobytes() == U.tobytes() and V2.tobytes() == V.tobytes()
    U3, _ = S.minpoly_vectors(n, K, seed + 1, p)
    assert p == 3 or U3.tobytes() != U.tobytes()


def test_argument_checks_that_fail_before_any_device(S):
    lib = S._abi.lib()
    err = S._abi.last_error
    words = 8
    coef = (C.c_int32 * words)(*([SENTINEL] * words))
    deg = C.c_int32(-7)
    buf = (C.c_int32 * words)(*([SENTINEL] * words))
    untouched = lambda: list(coef) == [SENTINEL] * words and list(buf) == [SENTINEL] * words and deg.value == -7

    # NULL handles
    assert lib.spasm_amd_krylov_sequence(None, 0, 1, 4, buf, 1, buf, 1, buf) == -1
    assert err() == "spasm_amd_krylov_sequence: NULL operator"
    assert lib.spasm_amd_krylov_sequence_dev(None, 0, 1, 4, buf, 1, buf, 1, buf, None) == -1
    assert err() == "spasm_amd_krylov_sequence_dev: NULL operator"
    assert lib.spasm_amd_minpoly(None, 8, 0, 0, None, None, coef, C.byref(deg)) == -1
    assert err() == "spasm_amd_minpoly: NULL matrix"
    assert lib.spasm_amd_spmv_minpoly(None, 8, 0, 0, None, None, coef, C.byref(deg)) == -1
    assert err() == "spasm_amd_spmv_minpoly: NULL operator"
    assert lib.spasm_amd_dcsr_minpoly(None, 8, 0, 0, None, None, coef, C.byref(deg)) == -1
    assert err() == "spasm_amd_dcsr_minpoly: NULL matrix"
    assert untouched()

    # a matrix that is not square
    tall = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)], []], 2, prime=127)
    assert lib.spasm_amd_minpoly(tall.data, 8, 0, 0, None, None, coef, C.byref(deg)) == -1
    assert err() == "spasm_amd_minpoly: not square (3 x 2)"
    with pytest.raises(S.SpasmError, match=r"not square \(3 x 2\)"):
        S.minpoly(tall)

    # K = 65 (and a negative K)
    sq = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)]], 2, prime=127)
    assert lib.spasm_amd_minpoly(sq.data, 65, 0, 0, None, None, coef, C.byref(deg)) == -1
    assert err() == "spasm_amd_minpoly: K out of range (0 <= K <= 64, 0 means 8)"
    assert lib.spasm_amd_minpoly(sq.data, -1, 0, 0, None, None, coef, C.byref(deg)) == -1 and "K out of range" in err()
    # NULL outputs, one vector without the other
    assert lib.spasm_amd_minpoly(sq.data, 2, 0, 0, None, None, None, C.byref(deg)) == -1 and err() == "spasm_amd_minpoly: NULL array"
    assert lib.spasm_amd_minpoly(sq.data, 2, 0, 0, buf, None, coef, C.byref(deg)) == -1
    assert err() == "spasm_amd_minpoly: U and V must both be given or both be NULL"
    assert untouched()

    # Berlekamp-Massey: ldc < len + 1, and the other checks of its arguments
    bm = lib.spasm_amd_berlekamp_massey
    assert bm(1, 4, buf, 1, 127, 0, coef, 4, C.byref(deg)) == -1
    assert err() == "spasm_amd_berlekamp_massey: ldc < len + 1"
    assert bm(2, 4, buf, 1, 127, 0, coef, 5, C.byref(deg)) == -1 and err() == "spasm_amd_berlekamp_massey: lds < count"
    assert bm(-1, 4, buf, 1, 127, 0, coef, 5, C.byref(deg)) == -1 and "count < 0" in err()
    assert bm(1, 4, buf, 1, 4294967296, 0, coef, 5, C.byref(deg)) == -1 and "prime out of range" in err()
    assert bm(1, 4, buf, 1, 127, 3, coef, 5, C.byref(deg)) == -1 and "where must be 0" in err()
    assert bm(1, 20224, buf, 1, 127, 1, coef, 20225, C.byref(deg)) == -1
    assert err() == "spasm_amd_berlekamp_massey: the LDS class does not fit (len = 20224, at most 20223)"
    assert bm(1, 4, None, 1, 127, 0, coef, 5, C.byref(deg)) == -1 and "NULL array" in err()
    assert untouched()
    # count == 0 succeeds without a device
    assert bm(0, 4, None, 0, 127, 0, None, 5, None) == 0 and err() == ""


def test_the_empty_matrix_has_the_polynomial_one_without_a_device(S):
    E = S.CSR.from_rows([], 0, prime=65521)
    assert S.minpoly(E).tolist() == [1]
    assert S._abi.last_error() == ""
