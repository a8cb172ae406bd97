"""The inputs shared by tests/test_block_solve_abi.py (CPU: the Python-integer reference decides every one of them at try 0) and
tests/test_gpu_block_solve.py (the device must then decide them the same way): matrices, right-hand sides and the seed."""
import functools

import numpy as np

import wiedemann_ref as W
from wiedemann_ref import bal

P3, P16, P32 = 3, 65521, 4294967291
SEED = 1                       # try 0 takes S.minpoly_vectors(n, b, SEED, p)
SHAPES = ((1, 2, 1), (7, 2, 2), (30, 4, 3), (33, 8, 8), (40, 16, 5))   # (n, b, K)
MID = ((130, 4, 4), (130, 16, 16))                                     # several chunks of the discrepancy, p = 65521
SINGULAR = (30, 4)             # (n, b): column 0 consistent, column 1 random


def terms(n, b):
    return 2 * -(-n // b) + 2


def dense_of(M):
    D = [[0] * M.m for _ in range(M.n)]
    for i in range(M.n):
        for k in range(int(M.ptr[i]), int(M.ptr[i + 1])):
            D[i][int(M.j[k])] += int(M.v[k])
    return D


@functools.lru_cache(maxsize=None)
def system(n, K, p, kind="random"):
    """(M, B): a sparse n x n matrix with a non-zero diagonal and up to 5 more entries a row, and n x K right-hand sides as
    balanced int32.  kind "singular": the last row is 2 * row 0 + 3 * row 1, column 0 of B is M x0 and column 1 is random."""
    rng = np.random.default_rng(1000 * n + 7 * K + p % 1009 + (kind == "singular"))
    D = np.zeros((n, n), dtype=np.int64)
    for i in range(n):
        cols = rng.choice(n, size=min(n, 5), replace=False)
        D[i, cols] = rng.integers(1, p, size=len(cols))
        D[i, i] = int(rng.integers(1, p))
    B = rng.integers(0, p, size=(n, K), dtype=np.int64)
    if kind == "singular":
        D[n - 1] = (D[0] * 2 + D[1] * 3) % p
        x0 = [int(x) for x in rng.integers(0, p, size=n)]
        B[:, 0] = [sum(int(a) * x for a, x in zip(row, x0)) % p for row in D]
    M = W.Mat.from_dense(D)
    return M, bal(B, p)


def np_block_sequence(M, U, V, length, p):
    """(length, b, b) residues in [0, p) by exact numpy int64 arithmetic (tests/test_gpu_block_wiedemann.py)"""
    Ur = np.asarray(U, dtype=np.int64) % p
    X = np.asarray(V, dtype=np.int64) % p
    b = Ur.shape[1]
    out = np.zeros((length, b, b), dtype=np.int64)
    for i in range(length):
        if i:
            X = M.apply(X, p)
        for r in range(b):
            out[i, r] = W.mulmod(np.broadcast_to(Ur[:, r:r + 1], X.shape).copy(), X, p).sum(axis=0) % p
    return out


def residual_is_zero(M, X, B, p, regular=True):
    """op = M: M X = B (or M X = 0) mod p in exact numpy products, column by column -> list of bools"""
    Xr = np.asarray(X, dtype=np.int64).reshape(M.n, -1) % p
    MX = M.apply(Xr, p)
    Br = np.asarray(B, dtype=np.int64).reshape(M.n, -1) % p if regular else np.zeros_like(MX)
    return [bool((MX[:, j] == Br[:, j]).all()) for j in range(MX.shape[1])]


SPECIAL = (("identity", 4, 3), ("identity", 2, 2), ("permutation", 2, 2), ("permutation", 16, 16))   # (kind, b, K), n = 40


@functools.lru_cache(maxsize=None)
def special(kind, K, p):
    """(M, B) of order 40: the identity, or a permutation with cycles 11, 7, 5, 5, 3, 3, 2, 2, 1, 1.  Their minimal polynomials
    have degree 1 and 2310 > n: the generator's degrees may sum to less than n, and the residual decides."""
    n = 40
    perm = list(range(n))
    if kind == "permutation":
        perm, at = [], 0
        for c in (11, 7, 5, 5, 3, 3, 2, 2, 1, 1):
            perm += [at + (k + 1) % c for k in range(c)]
            at += c
    M = W.Mat(n, n, np.arange(n + 1), np.array(perm), np.ones(n, dtype=np.int64))
    rng = np.random.default_rng(n + K + p % 1009)
    return M, bal(rng.integers(0, p, size=(n, K), dtype=np.int64), p)
