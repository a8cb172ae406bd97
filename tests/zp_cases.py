"""Inputs and exact references for the tests of the GF(p) primitives (csrc/zp.hpp): tests/test_zp_host.py runs the host compilation,
tests/test_gpu_zp.py the device and compares the two bit for bit.  The cases touch no library; every case is built once per
prime (lru_cache) and shared by the tests that use it, which must not modify the arrays.  The calls of the two host probes
(host_reduce, host_field) and the report of differing rows are here as well, since both test files use them.

References are Python integers where a product can pass 2^63 (the large primes) and numpy int64 where it cannot."""
import ctypes as C
import functools

import numpy as np


def is_prime(n):
    if n < 2:
        return False
    d = 2
    while d * d <= n:
        if n % d == 0:
            return False
        d += 1
    return True


def first_prime_above(n):
    """By trial division (2^31 + 11, in about 46 000 divisions)."""
    n += 1
    while not is_prime(n):
        n += 1
    return n


Q = first_prime_above(2**31)
# the small / general switch (2^16) on both sides, the sign bit of i32 on both sides, the largest accepted prime and its neighbour
PRIMES = [3, 5, 7, 127, 251, 257, 32749, 65519, 65521, 65537, 65539, 2**31 - 1, Q, 4294967279, 4294967291]
SMALL_PRIMES = [p for p in PRIMES if p < 65536]
LARGE_PRIMES = [p for p in PRIMES if p >= 65536]
EXHAUSTIVE_PRIMES = [3, 5, 7, 127, 251, 257, 1021]          # every pair of residues
INVERSE_PRIMES = [32749, 65519, 65521, 65537, 65539]        # every inverse


def halves(p):
    return p // 2, p // 2 - p + 1


def balanced(x, p):
    """Python integers."""
    r = x % p
    return r - p if r > p // 2 else r


def balanced_np(x, p):
    """numpy int64, exact while |x| < 2^63."""
    r = np.asarray(x, dtype=np.int64) % p
    return np.where(r > p // 2, r - p, r)


# ---- zp_reduce ------------------------------------------------------------------------------------------------------------------

# zp_reduce alone also runs 479 and 503: at the primes of the list the quotient never gets more than 1.5 off inside the domain (their
# 1 / p and the spacing of the doubles next to the top happen to round kindly); at these two the second correction does work.
REDUCE_PRIMES = PRIMES + [479, 503]


def reduce_top(p):
    """The domain of zp_reduce as the header of zp.hpp derives it: |x| <= min(3 * 2^51 * p, 2^62)."""
    return min(3 * 2**51 * p, 2**62)


@functools.lru_cache(maxsize=None)
def reduce_case(p):
    """(x as int64, the balanced residues as int32 from Python's % on Python integers), all x inside the domain:
    +-(2^k - 1), +-2^k, +-(2^k + 1) for every k up to the top; m p + r for r at and just past the two ends of the balanced range,
    0 and +-1, with m p near 2^31, 2^40, 2^48, 2^52, the top and half the top, in both signs; +-top itself; 20 000 random values
    log-uniform in magnitude (a uniform bit length, then uniform in that octave); and 4096 more in the upper half of the domain,
    where alone the quotient can be 2 off and the second correction of zp_reduce does any work."""
    half, mhalf = halves(p)
    top = reduce_top(p)
    vals = [0, top, -top]
    k = 1
    while 2**k - 1 <= top:
        for v in (2**k - 1, 2**k, 2**k + 1):
            vals += [v, -v]
        k += 1
    for T in (2**31, 2**40, 2**48, 2**52, top // 2, top - p, top):
        for m in {T // p, T // p + 1}:
            for r in (half, half + 1, mhalf, mhalf - 1, 0, 1, -1):
                vals += [m * p + r, -m * p + r]
    vals = [v for v in vals if abs(v) <= top]
    rng = np.random.default_rng(1000 + p % 99991)
    bits = rng.integers(1, top.bit_length() + 1, size=20000)
    lo = np.left_shift(np.int64(1), bits - 1)
    mag = rng.integers(lo, np.minimum(lo + (lo - 1), top), endpoint=True, dtype=np.int64)  # the last octave ends at the top
    rnd = mag * rng.choice(np.array([-1, 1], dtype=np.int64), size=mag.size)
    edge = rng.integers(top // 2, top, endpoint=True, size=4096, dtype=np.int64) * rng.choice(np.array([-1, 1], dtype=np.int64), size=4096)
    x = np.concatenate([np.asarray(vals, dtype=np.int64), rnd, edge])
    assert int(np.abs(x).max()) == top
    want = np.asarray([balanced(int(v), p) for v in x], dtype=np.int32)
    return x, want


# ---- field operations: the columns of spasm_amd_zp_probe ---------------------------------------------------------------------------

def inverse_table(p):
    """inv[a - mhalfp] = the balanced inverse of the residue a from Python's pow(a, -1, p); 0 for a = 0."""
    half, mhalf = halves(p)
    return np.asarray([balanced(pow(a, -1, p), p) if a else 0 for a in range(mhalf, half + 1)], dtype=np.int64)


def field_reference(p, a, b, c, inv):
    """The eight columns of spasm_amd_zp_probe for residues of a prime below 2^20 (64 a b < 2^63), numpy int64."""
    a, b, c = (np.asarray(v, dtype=np.int64) for v in (a, b, c))
    ab = a * b
    cols = [ab, ab + c, a + b, a - b, -a]
    out = [balanced_np(v, p) for v in cols] + [inv, balanced_np(ab, p), balanced_np(64 * ab, p)]
    return np.stack(out, axis=1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def exhaustive_case(p):
    """Every pair (a, b) of residues, c running through the residues cyclically; (a, b, c, the 8 expected columns)."""
    assert p <= 1021
    half, mhalf = halves(p)
    res = np.arange(mhalf, half + 1, dtype=np.int64)
    a = np.repeat(res, p)
    b = np.tile(res, p)
    c = res[(np.arange(p * p) * 7 + 3) % p]
    inv = inverse_table(p)[a - mhalf]
    want = field_reference(p, a, b, c, inv)
    return a.astype(np.int32), b.astype(np.int32), c.astype(np.int32), want


@functools.lru_cache(maxsize=None)
def inverse_case(p):
    """Every non-zero residue a with an arbitrary b and c; (a, b, c, expected inverse)."""
    half, mhalf = halves(p)
    a = np.concatenate([np.arange(mhalf, 0, dtype=np.int64), np.arange(1, half + 1, dtype=np.int64)])
    rng = np.random.default_rng(p)
    b = rng.integers(mhalf, half, endpoint=True, size=a.size)
    c = rng.integers(mhalf, half, endpoint=True, size=a.size)
    want = inverse_table(p)[a - mhalf]
    return a.astype(np.int32), b.astype(np.int32), c.astype(np.int32), want.astype(np.int32)


# ---- worst-case quotients at the large primes ----------------------------------------------------------------------------------

def quotient_targets(p):
    half, mhalf = halves(p)
    return [half, -half, half - 1, 1 - half, mhalf, 1, -1, 0]


@functools.lru_cache(maxsize=None)
def quotient_case(p):
    """20 000 random non-zero a; for each target t, b = t / a, so that a b is congruent to t: a product whose quotient a b / p has a
    fraction next to one half (t = +-halfp, +-(halfp - 1), mhalfp) or next to 0 (t = +-1, 0).  Every pair meets c in
    {0, 1, -1, halfp, mhalfp} and the c that puts a b + c on each target.  The congruence a b = t is checked here in Python
    integers (a b passes 2^63); with it the expected results are balanced(t) and balanced(t + c), which numpy int64 holds.
    Returns a dict: a, b, c and want (mul, axpy, add, sub, neg, inverse) with one row per vector, 13 per pair, and the pairs
    alone as pa, pb, pt."""
    assert p > 65536
    half, mhalf = halves(p)
    rng = np.random.default_rng(p % 1000003)
    a0 = rng.integers(mhalf, half, endpoint=True, size=20000)
    a0[a0 == 0] = 1
    targets = quotient_targets(p)
    a2, b2, t2, i2 = [], [], [], []
    for a in a0.tolist():
        ai = pow(a, -1, p)
        for t in targets:
            b = balanced(t * ai, p)
            assert (a * b - t) % p == 0 and mhalf <= b <= half
            a2.append(a); b2.append(b); t2.append(t); i2.append(balanced(ai, p))
    a2, b2, t2, i2 = (np.asarray(v, dtype=np.int64) for v in (a2, b2, t2, i2))
    tb = balanced_np(t2, p)
    cs = [np.full(a2.size, v, dtype=np.int64) for v in (0, 1, -1, half, mhalf)] + [balanced_np(t - tb, p) for t in targets]
    t = np.tile(tb, len(cs))
    c = np.concatenate(cs)
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)  # noqa: E731
    a, b = np.tile(a2, len(cs)), np.tile(b2, len(cs))
    want = np.stack([t, balanced_np(t + c, p), balanced_np(a + b, p), balanced_np(a - b, p), balanced_np(-a, p), np.tile(i2, len(cs))], axis=1)
    return {"a": i32(a), "b": i32(b), "c": i32(c), "want": i32(want), "pa": i32(a2), "pb": i32(b2), "pt": tb}


# ---- the host probes and the report, shared by the two test files -----------------------------------------------------------------

P32 = C.POINTER(C.c_int32)
P64 = C.POINTER(C.c_int64)


def host_reduce(S, p, x):
    out = np.full(x.size, 0x55555555, dtype=np.int32)
    rc = S._abi.lib().spasm_amd_zp_reduce_probe(p, 0, x.size, x.ctypes.data_as(P64), out.ctypes.data_as(P32))
    assert rc == 0, S._abi.last_error()
    return out


def host_field(S, p, a, b, c):
    out = np.full(6 * a.size, 0x55555555, dtype=np.int32)
    rc = S._abi.lib().spasm_amd_zp_field_probe_host(p, a.size, a.ctypes.data_as(P32), b.ctypes.data_as(P32), c.ctypes.data_as(P32), out.ctypes.data_as(P32))
    assert rc == 0, S._abi.last_error()
    return out.reshape(a.size, 6)


def report(name, p, got, want, *inputs):
    """The first few rows that differ, with their inputs; the number that differ."""
    bad = np.flatnonzero((got != want).reshape(got.shape[0], -1).any(axis=1))
    print(f"{name} p = {p}: {got.shape[0]} vectors, {bad.size} wrong: " + "; ".join(
        f"in {[int(v[i]) for v in inputs]} got {np.atleast_1d(got[i]).tolist()} want {np.atleast_1d(want[i]).tolist()}" for i in bad[:6]))
    return bad.size
