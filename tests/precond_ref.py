"""Host reference of preconditioned Wiedemann (tests/test_precond_abi.py, tests/test_gpu_precond.py), on top of wiedemann_ref.py:
the diagonal generator of the header in Python integers, the two preconditioned sequences, rank and determinant per try exactly
as the engine's driver takes them, and a plain Gaussian elimination mod p in Python integers for the true rank and determinant.
Nothing here touches a device."""
import numpy as np

from wiedemann_ref import Mat, bal, mulmod, plcm, ref_bm

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


def splitmix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def vectors(n, K, seed, p):
    """U, V of spasm_amd_minpoly_vectors as (n, K) arrays of residues in [0, p)"""
    out = []
    for t in range(2):
        w = [splitmix((seed + GOLD * (2 * e + t + 1)) & M64) % p for e in range(n * K)]
        out.append(np.array(w, dtype=np.int64).reshape(n, K))
    return out


def diagonal(length, seed, which, p):
    """word (which, i) = 1 + P_b(i mod N), N = p - 1, b = i div N; P_b: four Feistel rounds on two halves of h bits,
    (L, R) <- (R, L xor (splitmix64(seed + GOLD * ((which + 1) * 2^60 + b * 2^20 + r * 2^16 + R)) & (2^h - 1))), walked along its
    cycle until the result is below N; which = 1: the square of the word mod p.  Python integers in [1, p)."""
    N = p - 1
    h = max(1, ((N - 1).bit_length() + 1) // 2)
    mask = (1 << h) - 1
    out = []
    for i in range(length):
        base = ((which + 1) << 60) + ((i // N) << 20)
        x = i % N
        while True:
            L, Rr = x >> h, x & mask
            for r in range(4):
                L, Rr = Rr, L ^ (splitmix((seed + GOLD * (base + (r << 16) + Rr)) & M64) & mask)
            x = (L << h) | Rr
            if x < N:
                break
        w = 1 + x
        out.append(w * w % p if which == 1 else w)
    return out


def _col(d, p):
    return (np.array([int(x) % p for x in d], dtype=np.int64))[:, None]


def sequence(M, mode, d_left, d_right, U, V, length, p):
    """S[i, c] = sum_r U[r, c] (B^i V)[r, c] mod p as balanced int32, (length, K); mode 0: B = diag(d_left) A; mode 1:
    B = diag(d_right) A^T diag(d_left) A.  Any integers."""
    dim = M.m if mode else M.n
    Ur = np.asarray(U, dtype=np.int64).reshape(dim, -1) % p
    W = np.asarray(V, dtype=np.int64).reshape(dim, -1) % p
    dl = _col(d_left, p)
    T = M.transpose() if mode else None
    dr = _col(d_right, p) if mode else None
    out = np.zeros((length, Ur.shape[1]), dtype=np.int64)
    for i in range(length):
        if i:
            W = mulmod(np.broadcast_to(dl, (M.n, W.shape[1])), M.apply(W, p), p)
            if mode:
                W = mulmod(np.broadcast_to(dr, (M.m, W.shape[1])), T.apply(W, p), p)
        out[i] = mulmod(Ur, W, p).sum(axis=0) % p
    return bal(out, p)


class Refused(Exception):
    pass


def _split(f):
    e = 0
    while f[e] == 0:
        e += 1
    return e, len(f) - 1 - e


def try_poly(M, mode, K, seed, length, md, p):
    """(f, d_left): the lcm over the K projections of one try, as the driver takes it"""
    dim = M.m if mode else M.n
    U, V = vectors(dim, K, seed, p)
    dl = diagonal(M.n, seed, 0, p)
    dr = diagonal(M.m, seed, 1, p) if mode else None
    S = sequence(M, mode, dl, dr, U, V, length, p)
    polys = []
    for c in range(K):
        f, L = ref_bm(S[:, c], p)
        if _split(f)[1] > md:
            raise Refused("degree bound too small")
        polys.append(f)
    f = plcm(polys, p)
    if _split(f)[1] > md:
        raise Refused("degree bound too small")
    return f, dl


def rank(M, p, K=8, seed=0, tries=3, maxdeg=None):
    """(rank, certain, tries used) of wiedemann_rank"""
    mn = min(M.n, M.m)
    if mn == 0:
        return 0, True, 0
    md = mn if maxdeg is None or maxdeg <= 0 or maxdeg > mn else maxdeg
    best, used = -1, 0
    for t in range(tries):
        if best >= mn:
            break
        f, _ = try_poly(M, 1, K, seed + t, 2 * md + 2, md, p)
        best = max(best, _split(f)[1])
        used += 1
    return best, best == mn, used


def det(M, p, K=8, seed=0, tries=3):
    """(det as a balanced residue, status, tries used) of wiedemann_det"""
    n = M.n
    if n == 0:
        return 1, 1, 0
    for t in range(tries):
        f, d = try_poly(M, 0, K, seed + t, 2 * n, n, p)
        if f[0] == 0:
            return 0, 1, t + 1
        if len(f) - 1 == n:
            prod = 1
            for w in d:
                prod = prod * w % p
            v = f[0] * pow(prod, -1, p) % p
            if n & 1:
                v = (-v) % p
            return (v - p if v > p // 2 else v), 1, t + 1
    return 0, 0, tries


def eliminate(D, p):
    """(rank, det) of the dense matrix D (any integers) by Gaussian elimination mod p in Python integers; det is a residue in
    [0, p) and None when D is not square"""
    A = [[int(x) % p for x in row] for row in np.asarray(D, dtype=object).tolist()]
    n = len(A)
    m = len(A[0]) if n else 0
    r, d = 0, 1
    for c in range(m):
        piv = next((i for i in range(r, n) if A[i][c]), None)
        if piv is None:
            continue
        if piv != r:
            A[piv], A[r] = A[r], A[piv]
            d = -d
        d = d * A[r][c] % p
        inv = pow(A[r][c], -1, p)
        for i in range(r + 1, n):
            if A[i][c]:
                f = A[i][c] * inv % p
                A[i] = [(x - f * y) % p for x, y in zip(A[i], A[r])]
        r += 1
    if n != m:
        return r, None
    return r, (d % p if r == n else 0)
