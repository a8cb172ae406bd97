"""The device's GF(p) arithmetic (csrc/zp.hpp) against Python integers, edge values included.

Reference: src/SpaSM.jl:73-76 (field), :83-88 (balanced representatives), :383-390 (add, sub, mul, inverse, axpy by the
float-quotient formula).  Every result must be THE balanced residue in [p//2 - p + 1, p//2]."""
import ctypes as C

import numpy as np
import pytest
import zp_cases as Z
from test_gpu_accumulators import lazy_capacity
from zp_cases import P32, P64, host_field, host_reduce, report

pytestmark = pytest.mark.gpu

PRIMES = [3, 127, 42013, 65521, 65537, 2**31 - 1, 0xFFFFFFFB]


def balanced(x, p):
    r = x % p
    return r - p if r > p // 2 else r


@pytest.mark.parametrize("p", PRIMES)
def test_device_field_arithmetic_edge_values(S, p):
    lib = S._abi.lib()
    half, mhalf = p // 2, p // 2 - p + 1
    edge = sorted({v for v in (0, 1, -1, 2, -2, half, half - 1, mhalf, mhalf + 1, half // 2, -(half // 2), 3, -3) if mhalf <= v <= half})
    rng = np.random.default_rng(p % 1000003)
    rnd = [int(v) for v in rng.integers(mhalf, half + 1, size=200)]
    vals = edge + rnd
    a, b, c = [], [], []
    for x in edge:
        for y in edge:
            a.append(x); b.append(y); c.append(edge[(len(a) * 7) % len(edge)])
    for i in range(0, len(rnd) - 2, 1):
        a.append(rnd[i]); b.append(rnd[i + 1]); c.append(rnd[i + 2])
    n = len(a)
    A = np.asarray(a, dtype=np.int32); B = np.asarray(b, dtype=np.int32); Cc = np.asarray(c, dtype=np.int32)
    out = np.empty(8 * n, dtype=np.int32)
    P = C.POINTER(C.c_int32)
    rc = lib.spasm_amd_zp_probe(p, n, A.ctypes.data_as(P), B.ctypes.data_as(P), Cc.ctypes.data_as(P), out.ctypes.data_as(P))
    assert rc == 0, S._abi.last_error()
    out = out.reshape(n, 8)
    for i in range(n):
        x, y, z = a[i], b[i], c[i]
        want = [balanced(x * y, p), balanced(x * y + z, p), balanced(x + y, p), balanced(x - y, p), balanced(-x, p),
                balanced(pow(x, -1, p), p) if x % p else 0, balanced(x * y, p), balanced(64 * x * y, p)]
        assert out[i].tolist() == want, (p, x, y, z, out[i].tolist(), want)
        assert all(mhalf <= v <= half for v in out[i].tolist())


# ---- the primitives over their whole stated domain (tests/zp_cases.py; the host runs of the same cases: tests/test_zp_host.py) ------
# |zp_small_lazy| <= halfp + LAZY_SLACK is what zp_lazy_terms (csrc/zp.hpp) divides 2^31 - 1 by; read back from the capacity of
# p = 65521, where the division is exact to the unit: (2^31 - 1) // 65043 = 33016 = 32760 + 256
LAZY_SLACK = (2**31 - 1) // lazy_capacity(65521) - 65521 // 2
SCAN_CHUNK = 65536


def device_field(S, p, a, b, c):
    out = np.full(8 * a.size, 0x55555555, dtype=np.int32)
    rc = S._abi.lib().spasm_amd_zp_probe(p, a.size, a.ctypes.data_as(P32), b.ctypes.data_as(P32), c.ctypes.data_as(P32), out.ctypes.data_as(P32))
    assert rc == 0, S._abi.last_error()
    return out.reshape(a.size, 8)


def device_lazy(S, p, a, b):
    out = np.full(a.size, 0x5555555555555555, dtype=np.int64)
    rc = S._abi.lib().spasm_amd_zp_lazy_probe(p, a.size, a.ctypes.data_as(P32), b.ctypes.data_as(P32), out.ctypes.data_as(P64))
    assert rc == 0, S._abi.last_error()
    return out


def device_small_lazy(S, p, x):
    out = np.full(x.size, 0x55555555, dtype=np.int32)
    rc = S._abi.lib().spasm_amd_zp_small_lazy_probe(p, x.size, x.ctypes.data_as(P32), out.ctypes.data_as(P32))
    assert rc == 0, S._abi.last_error()
    return out


@pytest.mark.parametrize("p", Z.REDUCE_PRIMES)
def test_device_reduce_over_its_domain(S, p):
    """zp_reduce on the device over |x| <= min(3 * 2^51 * p, 2^62) (the header of zp.hpp): the inputs of Z.reduce_case, expected
    Python's % on Python integers; and the same bytes as the host compilation of the function."""
    x, want = Z.reduce_case(p)
    got = np.full(x.size, 0x55555555, dtype=np.int32)
    rc = S._abi.lib().spasm_amd_zp_reduce_probe(p, 1, x.size, x.ctypes.data_as(P64), got.ctypes.data_as(P32))
    assert rc == 0, S._abi.last_error()
    half, mhalf = Z.halves(p)
    assert report("device zp_reduce", p, got, want, x) == 0
    assert got.min() >= mhalf and got.max() <= half
    assert got.tobytes() == host_reduce(S, p, x).tobytes()


@pytest.mark.parametrize("p", Z.EXHAUSTIVE_PRIMES)
def test_device_field_operations_every_pair(S, p):
    """All eight columns of spasm_amd_zp_probe for EVERY pair (a, b) of residues, c cyclic, against numpy int64 (64 a b < 2^26) and
    an inverse table from Python's pow(a, -1, p); the first six are the host compilation's bytes."""
    a, b, c, want = Z.exhaustive_case(p)
    got = device_field(S, p, a, b, c)
    half, mhalf = Z.halves(p)
    assert report("device field", p, got, want, a, b, c) == 0
    assert got.min() >= mhalf and got.max() <= half
    assert np.ascontiguousarray(got[:, :6]).tobytes() == host_field(S, p, a, b, c).tobytes()


@pytest.mark.parametrize("p", Z.INVERSE_PRIMES)
def test_device_every_inverse(S, p):
    """zp_inverse of all p - 1 non-zero residues around the small / general switch."""
    a, b, c, want = Z.inverse_case(p)
    got = device_field(S, p, a, b, c)
    assert report("device inverse", p, got[:, 5], want, a) == 0
    assert np.ascontiguousarray(got[:, :6]).tobytes() == host_field(S, p, a, b, c).tobytes()


@pytest.mark.parametrize("p", Z.LARGE_PRIMES)
def test_device_worst_case_quotients(S, p):
    """zp_mul, zp_axpy and the i64 lazy product where (double)a * (double)b is inexact and the quotient's fraction is next to one
    half (Z.quotient_case: a b on +-halfp, +-(halfp - 1), mhalfp, +-1, 0 for 20 000 random a; 13 values of c per pair).  Exact
    against Python integers, the host's bytes, and for the raw lazy term t of ZpAcc<false>::mul_lazy: t congruent to a b and
    |t| <= 0.51 p, the bound its comment states.  Prints the largest |t| - halfp."""
    q = Z.quotient_case(p)
    got = device_field(S, p, q["a"], q["b"], q["c"])
    half, mhalf = Z.halves(p)
    assert report("device quotients", p, got[:, :6], q["want"], q["a"], q["b"], q["c"]) == 0
    assert np.ascontiguousarray(got[:, :6]).tobytes() == host_field(S, p, q["a"], q["b"], q["c"]).tobytes()
    # columns 6 and 7: the lazy product and 64 of them through acc_reduce_short; 64 t < 2^38
    assert (got[:, 6] == q["want"][:, 0]).all()
    assert (got[:, 7] == Z.balanced_np(64 * q["want"][:, 0].astype(np.int64), p)).all()
    t = device_lazy(S, p, q["pa"], q["pb"])
    excess = int(np.abs(t).max()) - half
    print(f"p = {p}: {t.size} raw i64 lazy terms, largest |t| - halfp = {excess}, 0.51 p - halfp = {51 * p // 100 - half}")
    # t = a b (mod p): a b is congruent to the target by construction (checked in Python integers), and |t - target| < 2^33
    assert ((t - q["pt"]) % p == 0).all()
    assert 100 * int(np.abs(t).max()) <= 51 * p


def scan(S, p, x_lo, x_hi):
    n = (x_hi - x_lo) // SCAN_CHUNK + 1
    tmax, tmin, bad = (np.full(n, 0x55555555, dtype=np.int32) for _ in range(3))
    rc = S._abi.lib().spasm_amd_zp_small_lazy_scan(p, x_lo, x_hi, SCAN_CHUNK, tmax.ctypes.data_as(P32), tmin.ctypes.data_as(P32), bad.ctypes.data_as(P32))
    assert rc == 0, S._abi.last_error()
    return tmax, tmin, bad


@pytest.mark.parametrize("p", Z.SMALL_PRIMES)
def test_device_small_lazy_bound_over_every_product(S, p):
    """|zp_small_lazy(x)| <= halfp + 256 -- the constant in zp_lazy_terms, hence in the capacity 65043 of an i32 accumulator, the
    Berlekamp-Massey length limit and the SpMV segment -- at EVERY x of [-halfp^2, halfp^2]: a superset of the products of two
    residues (ZpAcc<true>::mul_lazy is zp_small_lazy of the exact __mul24).  The device reports per chunk of 65536 values the
    largest and the smallest term and the number of terms not congruent to x (integer remainder).  The scan is then tied to
    values checked here: the raw terms of the chunks holding the global extremes, the first, the last, the one around 0 and 32
    seeded ones come back through spasm_amd_zp_small_lazy_probe and are judged in numpy int64, extremes included.  For
    p <= 257 every pair (a, b) goes through the lazy product itself and must give the term of x = a b.
    Prints the worst excess over halfp and where it is (DESIGN section 5 keeps the table)."""
    half, mhalf = Z.halves(p)
    x_lo, x_hi = -half * half, half * half
    tmax, tmin, bad = scan(S, p, x_lo, x_hi)
    worst = max(int(tmax.max()), -int(tmin.min()))
    kmax, kmin = int(tmax.argmax()), int(tmin.argmin())
    assert int(bad.sum()) == 0, np.flatnonzero(bad)[:8]
    n = tmax.size
    rng = np.random.default_rng(p)
    chunks = sorted({kmax, kmin, 0, n - 1, (0 - x_lo) // SCAN_CHUNK} | set(rng.integers(0, n, size=32).tolist()))
    lo = np.asarray([x_lo + k * SCAN_CHUNK for k in chunks], dtype=np.int64)
    ln = np.minimum(x_hi - lo + 1, SCAN_CHUNK)
    x = np.concatenate([np.arange(a, a + m, dtype=np.int64) for a, m in zip(lo, ln)])
    t = device_small_lazy(S, p, x.astype(np.int32)).astype(np.int64)
    assert ((t - x) % p == 0).all()
    starts = np.concatenate([[0], np.cumsum(ln)[:-1]])
    cmax, cmin = np.maximum.reduceat(t, starts), np.minimum.reduceat(t, starts)
    assert cmax.tolist() == tmax[chunks].tolist() and cmin.tolist() == tmin[chunks].tolist()
    i = int(np.abs(t).argmax())
    assert abs(int(t[i])) == worst  # the chunks of the global extremes are among those fetched
    print(f"p = {p}: {x_hi - x_lo + 1} values in {n} chunks, worst |t| - halfp = {worst - half} at x = {int(x[i])} (t = {int(t[i])}); "
          f"allowed {LAZY_SLACK}; p * 2^-9 = {p / 512:.1f}")
    assert int(np.abs(t).max()) <= half + LAZY_SLACK
    assert worst <= half + LAZY_SLACK
    if p <= 257:
        res = np.arange(mhalf, half + 1, dtype=np.int64)
        a, b = np.repeat(res, p), np.tile(res, p)
        via_mul = device_lazy(S, p, a.astype(np.int32), b.astype(np.int32))
        via_x = device_small_lazy(S, p, (a * b).astype(np.int32))
        assert (via_mul == via_x).all()
        assert ((via_mul - a * b) % p == 0).all() and int(np.abs(via_mul).max()) <= half + LAZY_SLACK


def test_small_lazy_probes_refuse_a_general_prime(S):
    """zp_small_lazy exists for p < 2^16 only: its two probes return an error for 65537 and for an x outside its domain."""
    lib = S._abi.lib()
    x = np.array([1, 2], dtype=np.int32)
    out = np.full(2, 0x55555555, dtype=np.int32)
    assert lib.spasm_amd_zp_small_lazy_probe(65537, 2, x.ctypes.data_as(P32), out.ctypes.data_as(P32)) == 1
    assert "2^16" in S._abi.last_error()
    assert lib.spasm_amd_zp_small_lazy_scan(65537, -4, 4, 2, out.ctypes.data_as(P32), out.ctypes.data_as(P32), out.ctypes.data_as(P32)) == 1
    assert "2^16" in S._abi.last_error()
    assert lib.spasm_amd_zp_small_lazy_scan(3, -(2**30) - 1, 0, SCAN_CHUNK, out.ctypes.data_as(P32), out.ctypes.data_as(P32), out.ctypes.data_as(P32)) == 1
    assert "domain" in S._abi.last_error()
    assert (out == 0x55555555).all()
