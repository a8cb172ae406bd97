"""Host references shared by tests/test_gpu_krylov.py and tests/test_gpu_minpoly.py: exact sparse products, projected Krylov
sequences, Berlekamp-Massey and Wiedemann's method in numpy int64 (products of two residues of a prime above 2^31 are taken in two
16-bit halves of one factor, as in tests/test_gpu_charpoly.py), and polynomial arithmetic over GF(p) in Python integers.  Nothing
here touches a device."""
import numpy as np

PRIMES = (3, 127, 65521, 2**31 - 1, 4294967291)


def bal(v, p):
    """integers (any array or list) -> the int32 array of their balanced residues, same shape"""
    a = np.asarray(v)
    if a.dtype == object:
        a = np.array([int(x) % p for x in a.ravel()], dtype=np.int64).reshape(a.shape)
    else:
        a = a.astype(np.int64) % p
    return np.where(a > p // 2, a - p, a).astype(np.int32)


def mulmod(a, b, p):
    """a * b mod p for int64 arrays of residues in [0, p), p < 2^32"""
    if p < 2**31:
        return a * b % p
    return ((a * (b >> 16) % p) * 65536 + a * (b & 0xFFFF)) % p


class Mat:
    """a square or rectangular CSR on the host: ptr, j, v with v any int64 (reduced where it is used)"""

    def __init__(self, n, m, ptr, j, v):
        self.n, self.m = n, m
        self.ptr = np.asarray(ptr, dtype=np.int64)
        self.j = np.asarray(j, dtype=np.int64)
        self.v = np.asarray(v, dtype=np.int64)

    @classmethod
    def from_dense(cls, D):
        D = np.asarray(D, dtype=np.int64)
        n, m = D.shape
        rows, cols = np.nonzero(D)
        ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(rows, minlength=n), out=ptr[1:])
        return cls(n, m, ptr, cols, D[rows, cols])

    @classmethod
    def from_rows(cls, rows, m):
        ptr = np.zeros(len(rows) + 1, dtype=np.int64)
        ptr[1:] = np.cumsum([len(r) for r in rows])
        j = np.array([c for r in rows for c, _ in r], dtype=np.int64)
        v = np.array([x for r in rows for _, x in r], dtype=np.int64)
        return cls(len(rows), m, ptr, j, v)

    def transpose(self):
        row = np.repeat(np.arange(self.n), np.diff(self.ptr))
        order = np.argsort(self.j, kind="stable")
        ptr = np.zeros(self.m + 1, dtype=np.int64)
        ptr[1:] = np.cumsum(np.bincount(self.j, minlength=self.m))
        return Mat(self.m, self.n, ptr, row[order], self.v[order])

    def csr(self, S, p, reduce=True):
        """the engine's CSR; reduce=False stores the values as they are (they must fit int32)"""
        return S.CSR.from_arrays(self.n, self.m, self.ptr, self.j, bal(self.v, p) if reduce else self.v, prime=p)

    def apply(self, X, p):
        """A X mod p, X (m, k) int64 residues in [0, p) -> (n, k) residues in [0, p).  A row sums at most len * p < 2^63."""
        Y = np.zeros((self.n, X.shape[1]), dtype=np.int64)
        ne = np.nonzero(np.diff(self.ptr))[0]
        if len(ne):
            v = self.v % p
            for c0 in range(0, X.shape[1], 16):
                prod = mulmod(v[:, None], X[self.j, c0:c0 + 16], p)
                Y[ne, c0:c0 + 16] = np.add.reduceat(prod, self.ptr[ne], axis=0) % p
        return Y


def ref_sequence(M, U, V, length, p, trans=False):
    """S[i, c] = sum_r U[r, c] (op(A)^i V)[r, c] mod p as balanced int32, (length, K)"""
    A = M.transpose() if trans else M
    Ur = np.asarray(U, dtype=np.int64).reshape(M.n, -1) % p
    W = np.asarray(V, dtype=np.int64).reshape(M.n, -1) % p
    out = np.zeros((length, Ur.shape[1]), dtype=np.int64)
    for i in range(length):
        if i:
            W = A.apply(W, p)
        out[i] = mulmod(Ur, W, p).sum(axis=0) % p   # n * p < 2^63
    return bal(out, p)


def ref_bm(s, p):
    """Berlekamp-Massey on the sequence s (any integers): (f, L) with f the monic x^L C(1/x), low degree first, residues in
    [0, p), as a list of Python integers.  The update rule of the textbook (Massey 1969): on a non-zero discrepancy d,
    C <- C - (d / b) x^m B; the length changes when 2 L <= i."""
    s = np.asarray(s, dtype=np.int64) % p
    N = len(s)
    C = np.zeros(N + 1, dtype=np.int64)
    B = np.zeros(N + 1, dtype=np.int64)
    C[0] = B[0] = 1
    L, LB, m, binv = 0, 0, 1, 1
    for i in range(N):
        d = int(mulmod(C[: L + 1], s[i - L: i + 1][::-1], p).sum() % p)
        if d == 0:
            m += 1
            continue
        f = np.int64(d * binv % p)
        if 2 * L <= i:
            T = C.copy()
            C[m: m + LB + 1] = (C[m: m + LB + 1] - mulmod(B[: LB + 1], f, p)) % p
            B, LB, L, binv, m = T, L, i + 1 - L, pow(d, -1, p), 1
        else:
            top = min(LB + m, N)
            C[m: top + 1] = (C[m: top + 1] - mulmod(B[: top - m + 1], f, p)) % p
            m += 1
    return [int(x) for x in C[: L + 1][::-1]], L


# ---- polynomials over GF(p) in Python integers: residues in [0, p), low degree first, no zero leading word ----
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
        if x:
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
        if f != r:
            r = pmonic(pdivmod(pmul(r, f, p), pgcd(r, f, p), p)[0], p)
    return r


def ref_minpoly(M, U, V, p):
    """Wiedemann on the host with the vectors U, V (n x K): the lcm of the Berlekamp-Massey polynomials of the K projected
    sequences of 2 n terms, as residues in [0, p)"""
    seq = ref_sequence(M, U, V, 2 * M.n, p)
    return plcm([ref_bm(seq[:, c], p)[0] for c in range(seq.shape[1])], p)


def poly_apply(op, f, V, p):
    """f(A) V mod p through op.apply (Horner), V (n, K) int32; f residues in [0, p) or balanced"""
    fb = [int(x) for x in bal(np.array([int(x) for x in f], dtype=object), p)]
    Vl = np.asarray(V, dtype=np.int64)
    R = bal(Vl * fb[-1], p)   # |v * c| < 2^62
    for c in fb[-2::-1]:
        R = op.apply(np.ascontiguousarray(R), bal(Vl * c, p))   # R <- A R + c V
    return R


def companion(f, p):
    """the companion matrix (dense, int64) of the monic f = f[0] + f[1] x + .. + x^d: its minimal and characteristic polynomial"""
    d = len(f) - 1
    D = np.zeros((d, d), dtype=np.int64)
    for i in range(1, d):
        D[i, i - 1] = 1
    for i in range(d):
        D[i, d - 1] = (-int(f[i])) % p
    return D


def block_diag(blocks):
    n = sum(len(b) for b in blocks)
    D = np.zeros((n, n), dtype=np.int64)
    at = 0
    for b in blocks:
        D[at: at + len(b), at: at + len(b)] = b
        at += len(b)
    return D


def rand_monic(rng, d, p):
    return [int(x) for x in rng.integers(0, p, size=d)] + [1]


def lfsr_sequence(f, init, count, p):
    """count terms of the sequence with s[i + d] = -sum_j f[j] s[i + j] that starts with init (d terms)"""
    d = len(f) - 1
    s = np.zeros(max(count, d), dtype=np.int64)
    s[:d] = np.asarray(init, dtype=np.int64) % p
    nf = (-np.asarray(f[:d], dtype=object)) % p
    nf = np.array([int(x) for x in nf], dtype=np.int64)
    for i in range(count - d):
        s[i + d] = mulmod(nf, s[i: i + d], p).sum() % p
    return s[:count]
