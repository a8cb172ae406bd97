"""Designed inputs and exact references for the dense finishes (csrc/dense.hpp, csrc/dense_tall.hpp, the f64 panels and the rank-1
updates of csrc/kernels.hpp, their host side in engine.hip): matrices whose whole elimination is known in closed form and whose
block updates sum K products of EQUAL sign and largest magnitude -- what random residues (partial sums ~ sqrt(K) p) never do.

Pure numpy and Python integers: neither the library nor torch is imported, so that test_dense_bounds_host.py proves every
construction on a machine without a GPU and test_gpu_dense_bounds.py takes them for granted.

The constants restated here, with their sources:
  engine.hip, dense_elem_bytes / dense_eliminate_i8   one base-256 digit and bytes for p <= 255, two digits and shorts for p < 2^16
  engine.hip, dense_eliminate_i8     block of KB = 1024 columns (SPASM_AMD_DENSE_KB: 64 .. 2048), panels of DP_W = 64
  dense.hpp, k_gemm_i8               one digit: |acc| <= K * 127^2 < 2^25 for K <= 2048, then zp_small_lazy and one correction
  dense.hpp, zp_digits               v > 32639 goes to v - p: representatives in [-32896, 32639], both digits signed bytes
  engine.hip, dense_eliminate        ints and f64 panels of DPB = 64 columns for 2^16 <= p <= 2^24 ("64 (p/2)^2 < 2^53"), rank-1
                                     updates above
  dense_tall.hpp, TallWork           the rows beyond the first slab are reduced KB = 1024 pivots at a time

The construction.  K = the block width under test, h = p // 2, l[s] and u[s] balanced residues (s < K), E an r x c remainder.
  Ut   K x (K + c): Ut[s][s] = 1, Ut[s][j] = u[s] for j > s (`upper`) or for j >= K only (the left K x K part is the identity)
  Lm   (K + r) x K: Lm[s][s] = 1, Lm[i][s] = l[s] for i > s
  D  = Lm Ut mod p, plus E on the rows >= K and the columns >= K
Column s of Lm is constant below the diagonal, so row i of D is W_i + Ut[i] (i < K) or W_K (+ E) with W_i = sum_{s < i} l[s] Ut[s]:
a running sum, no matrix product.  Under the rule of the finish -- the pivot of a column is the first row, not yet a pivot, with a
non-zero in it -- row s wins column s for s < K (after the columns before it, row i >= s holds sum_{t >= s} Lm[i][t] Ut[t]: a 1 on
column s in row s, and the rows above are pivots already), its multipliers are Lm[i][s], its normalised row is Ut[s], and what is
left of the rows >= K after K pivots is E.  The update of the columns right of the block is then, for every row >= K and every
column, the sum of the K products l[s] u[s]."""
import functools

import numpy as np

DP_W = 64
KB_DEFAULT, KB_MAX = 1024, 2048
TALL_KB = 1024
DPB = 64
BAND_LO = 32639          # zp_digits: residues above this one take the negative representative
PATTERNS = ("pp", "pm", "mp", "mm", "alt")


def is_prime(n):
    """deterministic Miller-Rabin (the bases 2, 3, 5, 7 decide every n < 3 215 031 751; 11 and 13 carry it past 2^32)"""
    n = int(n)
    if n < 2:
        return False
    for q in (2, 3, 5, 7, 11, 13):
        if n % q == 0:
            return n == q
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def next_prime(n):
    """the smallest prime above n"""
    n = int(n) + 1
    while not is_prime(n):
        n += 1
    return n


def prev_prime(n):
    """the largest prime below n"""
    n = int(n) - 1
    while not is_prime(n):
        n -= 1
    return n


def bal(v, p):
    """balanced residues of an int64 / object array (or of one integer): in [p // 2 - p + 1, p // 2]"""
    if isinstance(v, (int, np.integer)):
        r = int(v) % p
        return r - p if 2 * r > p else r
    r = np.mod(v, p)
    return np.where(2 * r > p, r - p, r)


def zp_digits(v, p):
    """dense.hpp zp_digits in Python integers: (d0, d1) with d0 + 256 d1 congruent to v"""
    v = int(v)
    if v > BAND_LO:
        v -= p
    d0 = ((v + 128) & 255) - 128
    return d0, (v - d0) >> 8


def pattern_values(p, K, pattern):
    """(l, u): the multiplier of column s below the diagonal and the entry of the normalised pivot row s right of it.
    pp / pm / mp / mm: l = +-h, u = +-h throughout, so that the K products of an update are equal; alt: l = h, u = (-1)^s h, the
    same magnitudes cancelling in pairs; band (p > 65279): both run through 32639, 32640, h, -h and -32768 + p -- the two edges of
    the band zp_digits moves, the balanced extremes and the most negative representative -- l with s, u with s // 5, so that the K
    terms hold all 25 pairs and with them all four sign combinations of d0 d1 + d1 d0; minus2: l = u = -2, small as balanced
    residues and p - 2 (odd) as canonical ones -- 64 products (p - 2)^2 pass 2^53 from p ~ 2^23.5 and are odd, so a sum of canonical
    f64 operands rounds at every step beyond 2^53: the input for "exact in f64 ONLY for balanced operands"."""
    h = p // 2
    s = np.arange(K, dtype=np.int64)
    if pattern == "minus2":
        return np.full(K, -2, dtype=np.int64), np.full(K, -2, dtype=np.int64)
    if pattern == "alt":
        return np.full(K, h, dtype=np.int64), np.where(s % 2 == 0, h, -h).astype(np.int64)
    if pattern == "band":
        vals = np.array([bal(v, p) for v in (BAND_LO, BAND_LO + 1, h, -h, -32768 + p)], dtype=np.int64)
        return vals[s % 5], vals[(s // 5) % 5]
    sl, su = [{"p": 1, "m": -1}[ch] for ch in pattern]
    return np.full(K, sl * h, dtype=np.int64), np.full(K, su * h, dtype=np.int64)


def remainder(p, r, c, seed):
    """E: r x c balanced residues, uniformly random"""
    rng = np.random.default_rng(seed)
    return rng.integers(p // 2 - p + 1, p // 2 + 1, size=(r, c), dtype=np.int64)


def unit_rows(K, c, u, upper=True):
    """Ut (see the module's text), int64, balanced"""
    Ut = np.zeros((K, K + c), dtype=np.int64)
    Ut[:, K:] = u[:, None]
    if upper:
        Ut[:, :K] = np.triu(np.broadcast_to(u[:, None], (K, K)), 1)
    Ut[np.arange(K), np.arange(K)] = 1
    return Ut


def designed(p, K, r, c, pattern, seed=1, upper=True):
    """(D, Ut, E): the (K + r) x (K + c) input as balanced int64 residues, the K normalised pivot rows it must give, the remainder.
    Balanced operands keep l[s] Ut[s][j] below 2^62 for every prime up to 0xFFFFFFFB; the running sum is reduced at every step that
    could pass 2^62 (K terms below p / 2 each stay far below it)."""
    l, u = pattern_values(p, K, pattern)
    Ut = unit_rows(K, c, u, upper)
    E = remainder(p, r, c, seed)
    T = bal(l[:, None] * Ut, p)                 # l[s] Ut[s], a scaling of rows: |l|, |Ut| <= 2^31
    W = np.zeros((K + 1, K + c), dtype=np.int64)
    np.cumsum(T, axis=0, out=W[1:])             # W[i] = sum_{s < i}: at most 2048 terms below 2^31
    W = bal(W, p)
    D = np.empty((K + r, K + c), dtype=np.int64)
    D[:K] = W[:K] + Ut
    D[K:] = W[K]
    D[K:, K:] += E
    return bal(D, p), Ut, E


def eliminate(M, p, max_pivots=None):
    """The finish's elimination in exact integers: columns left to right, the pivot of a column is the first row, not yet a pivot,
    with a non-zero in it; its row is normalised and taken out of every row that is no pivot.  Returns (prow, pcol, U, M'): the pivot
    rows and columns in election order, the normalised pivot rows (balanced), the matrix after the last pivot taken (balanced; the
    pivot rows normalised).  The entries are Python integers (an object array) when a product of two residues could pass 2^62."""
    M = np.array(M, dtype=np.int64 if p < (1 << 31) else object) % p
    n, m = M.shape
    is_piv = np.zeros(n, dtype=bool)
    prow, pcol = [], []
    for c in range(m):
        if max_pivots is not None and len(prow) == max_pivots:
            break
        cand = np.flatnonzero((M[:, c] != 0) & ~is_piv)
        if cand.size == 0:
            continue
        k = int(cand[0])
        M[k] = M[k] * pow(int(M[k, c]), -1, p) % p
        is_piv[k] = True
        rows = np.flatnonzero((M[:, c] != 0) & ~is_piv)
        if rows.size:
            M[rows] = (M[rows] - M[rows, c][:, None] * M[k][None, :]) % p
        prow.append(k)
        pcol.append(c)
    M = bal(M, p)
    U = M[prow] if prow else M[:0]
    return prow, pcol, np.array(U.tolist(), dtype=np.int64), np.array(M.tolist(), dtype=np.int64)


def eliminate_plain(M, p):
    """the same rule with nothing but Python lists and integers (the host test holds eliminate() against it)"""
    M = [[int(v) % p for v in row] for row in M]
    n, m = len(M), len(M[0])
    is_piv = [False] * n
    prow, pcol = [], []
    for c in range(m):
        k = next((i for i in range(n) if not is_piv[i] and M[i][c]), None)
        if k is None:
            continue
        inv = pow(M[k][c], -1, p)
        M[k] = [v * inv % p for v in M[k]]
        is_piv[k] = True
        for i in range(n):
            if not is_piv[i] and M[i][c]:
                f = M[i][c]
                M[i] = [(a - f * b) % p for a, b in zip(M[i], M[k])]
        prow.append(k)
        pcol.append(c)
    return prow, pcol, [[bal(v, p) for v in M[k]] for k in prow]


def reduced_form(U, pcol, p):
    """the unique reduced row echelon form (balanced) from echelon rows U with unit pivots on the columns pcol, ascending"""
    R = np.array(U, dtype=np.int64 if p < (1 << 31) else object) % p
    for t in range(len(pcol) - 1, -1, -1):
        above = np.flatnonzero(R[:t, pcol[t]] != 0)
        if above.size:
            R[above] = (R[above] - R[above, pcol[t]][:, None] * R[t][None, :]) % p
    return np.array(bal(R, p).tolist(), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def remainder_echelon(p, r, c, seed):
    """(prow, pcol, U) of the remainder E of designed(p, ., r, c, ., seed)"""
    prow, pcol, U, _ = eliminate(remainder(p, r, c, seed), p)
    return prow, pcol, U


def expected(p, K, r, c, pattern, seed=1, upper=True):
    """What the finish must return for designed(...): (pivot columns ascending, the input row of each, the rows of U in that order)."""
    _, u = pattern_values(p, K, pattern)
    Ut = unit_rows(K, c, u, upper)
    prow, pcol, UE = remainder_echelon(p, r, c, seed)
    cols = list(range(K)) + [K + j for j in pcol]
    rows = list(range(K)) + [K + i for i in prow]
    U = np.zeros((K + len(pcol), K + c), dtype=np.int64)
    U[:K] = Ut
    U[K:, K:] = UE
    return cols, rows, U


def low_rank(p, n, m, rank, seed):
    """an n x m matrix of balanced residues of rank <= `rank`, a product of random factors (exact: Python integers above 2^31),
    with a zero column and a column that repeats an earlier one twice over, so that free columns sit among the pivots"""
    rng = np.random.default_rng(seed)
    dt = np.int64 if p < (1 << 31) else object
    A = rng.integers(0, p, size=(n, rank), dtype=np.int64).astype(dt)
    B = rng.integers(0, p, size=(rank, m), dtype=np.int64).astype(dt)
    M = np.zeros((n, m), dtype=dt)
    for k in range(rank):                        # rank-1 terms reduced one by one: nothing passes 2^62
        M = (M + A[:, k][:, None] * B[k][None, :] % p) % p
    M[:, 5] = 0
    M[:, 70] = 2 * M[:, 3] % p
    return np.array(bal(M, p).tolist(), dtype=np.int64)


# ---- the bounds the GPU tests rely on, in Python integers ----------------------------------------------------------------------

def one_digit_sum(p, K):
    """largest |accumulator| of k_gemm_i8 with one digit: K products of two residues of magnitude h"""
    return K * (p // 2) ** 2


def two_digit_sums(p, K, l, u):
    """the three accumulators of k_gemm_i8 with two digits for the K products l[s] u[s], and their 64-bit recombination"""
    a0 = a1 = a2 = 0
    for x, y in zip(l[:K].tolist(), u[:K].tolist()):
        x0, x1 = zp_digits(x, p)
        y0, y1 = zp_digits(y, p)
        a0 += x0 * y0
        a1 += x0 * y1 + x1 * y0
        a2 += x1 * y1
    return a0, a1, a2, a0 + 256 * a1 + 65536 * a2


def f64_fma_chain(a, b, n):
    """the f64 value of acc = fma(-a, b, acc), n times from 0, rounding to nearest even at every step, and the exact -n a b: what
    k_panel_trsm2's chain returns for n equal products of the integers a and b (|a b| < 2^53)"""
    acc = 0
    for _ in range(n):
        exact = acc - a * b
        m = abs(exact)
        e = max(m.bit_length() - 53, 0)
        q, rem = m >> e, m & ((1 << e) - 1)
        half = (1 << e) >> 1
        if e and (rem > half or (rem == half and q & 1)):
            q += 1
        acc = (q << e) * (1 if exact >= 0 else -1)
    return acc, -n * a * b


def f64_panel_sum(p, balanced=True):
    """largest sum of the DPB = 64 products of one f64 panel update: operands of magnitude h (balanced) or p - 1 (canonical)"""
    v = p // 2 if balanced else p - 1
    return DPB * v * v
