"""Builders and exact references for the worst-case inputs of the two sparse exact-arithmetic families: the products with A
(csrc/spmv.hpp, spmv_launch / SpmvView::bin / apply_dev in engine.hip) and the matrix algebra (csrc/spgemm.hpp, spg_run).

Pure numpy and Python integers: neither the library nor torch is imported, so that test_sparse_worst_cases_host.py can prove every
construction on a machine without a GPU, and the GPU tests (test_gpu_spmv_bounds.py, test_gpu_algebra_bounds.py) take them for
granted.

The constants restated here, with their sources:
  spmv.hpp:22      SPMV_SHORT = 32      rows up to this length go to the short-row teams
  spmv.hpp:23      SPMV_SEG = 16384     longest row one wave takes whole; longer rows are cut into segments of this length
  spmv.hpp:26      spmv_short_team(kw) = min(64, 8 kw); a team is (E = TEAM / KW entries) x (KW columns), medium / long: TEAM = 64
  engine.hip, spasm_amd_spmv::apply_dev   a block of k columns goes in chunks of 64; a chunk of `rem` columns runs the kernel of width
                   kw = the power of two >= rem (at most 64), with kc = min(rem, kw) columns live
  spgemm.hpp:43    SPG_TINY = 32        rows with at most this many products go to the team kernel (16 lanes a row, 16 rows a workgroup)
  spgemm.hpp:97    spg_class_of(bound)  9 for bound <= 0, 0 for bound <= 32, 1 + c for bound <= 64 << c (c = 0 .. 6), else 8 (global)
  spgemm.hpp:297   a hash class c has a table of 2^LOGT slots, LOGT = 7 + c, and a list of LIST = 2^(LOGT - 1) live entries
  engine.hip, spg_launch_class            64 lanes (= segments per batch, BS) up to LOGT 10, 256 above; the global class: 256
  spgemm.hpp:317   home slot of column c: ((uint32)c * 2654435761) >> (32 - LOGT); the probe goes on at (h + 1) & (SLOTS - 1)
  zp.hpp:35        F.small = p < 65536: i32 lazy terms, |term| <= p/2 + 256 (zp_small_lazy, zp.hpp:112); i64 terms otherwise

A matrix is a Mat (n, m, ptr, j, v): CSR arrays in int64, columns in stored order."""
import functools
from typing import NamedTuple

import numpy as np

INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1

SPMV_SHORT, SPMV_SEG = 32, 16384
SPG_TINY, SPG_TINY_TEAM = 32, 16
SPG_LOGT_MIN, SPG_LOGT_MAX = 7, 13
SPG_CLS_GLOBAL, SPG_CLS_EMPTY = 8, 9

# SpMV: row lengths on both sides of 32 | 33 and 16384 | 16385, a last segment of one entry (2 SPMV_SEG + 1), interleaved so that
# the short, the medium and the long list all have holes (short_all is false)
SPMV_LENGTHS = [33, 0, 16385, 1, 64, 31, 32768, 32, 16383, 63, 32769, 65, 16384]
SPMV_BLOCKS = [1, 2, 3, 4, 5, 8, 16, 17, 32, 33, 63, 64, 65, 128, 129]
# sparse algebra: 32 | 33 (tiny | hash), 64 << c | (64 << c) + 1 (hash class c + 1 | the next), 4096 | 4097 (hash | global)
SPG_EDGES = [32] + [64 << c for c in range(SPG_LOGT_MAX - SPG_LOGT_MIN + 1)]
SPG_M = 8192


class Mat(NamedTuple):
    n: int
    m: int
    ptr: np.ndarray
    j: np.ndarray
    v: np.ndarray


def mat_from_rows(rows, m):
    """rows[i] = (columns, values) in stored order"""
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(c) for c, _ in rows])
    j = np.concatenate([np.asarray(c, dtype=np.int64) for c, _ in rows] + [np.zeros(0, np.int64)])
    v = np.concatenate([np.asarray(x, dtype=np.int64) for _, x in rows] + [np.zeros(0, np.int64)])
    assert len(j) == len(v) == ptr[-1] and (len(j) == 0 or (j.min() >= 0 and j.max() < m))
    assert len(v) == 0 or (v.min() >= INT32_MIN and v.max() <= INT32_MAX)
    return Mat(len(rows), int(m), ptr, j, v)


def row_lengths(M):
    return np.diff(M.ptr)


def bal(v, p):
    """balanced residues of an int64 array (or one integer)"""
    if isinstance(v, (int, np.integer)):
        r = int(v) % p
        return r - p if 2 * r > p else r
    r = np.asarray(v, dtype=np.int64) % p
    return np.where(2 * r > p, r - p, r)


def rand_values(p, count, rng):
    """random balanced residues, none zero"""
    return bal(rng.integers(1, p, size=count, dtype=np.int64), p)


def rand_int32(rng, shape):
    """any int32, with INT32_MIN and INT32_MAX placed in the first column"""
    a = rng.integers(INT32_MIN, INT32_MAX + 1, size=shape, dtype=np.int64).astype(np.int32)
    if a.shape[0] >= 2:
        a[0, 0], a[1, 0] = INT32_MIN, INT32_MAX
        a[-1, -1], a[-2, -1] = INT32_MAX, INT32_MIN
    return a


# ---- restated rules ---------------------------------------------------------------------------------------------------------
def spmv_team(kw):
    return min(64, 8 * kw)


def spmv_chunks(k):
    """(kw, kc) of every launch apply_dev makes for a block of k columns"""
    out = []
    for k0 in range(0, k, 64):
        rem, kw = k - k0, 1
        while kw < rem and kw < 64:
            kw <<= 1
        out.append((kw, min(rem, kw)))
    return out


def spmv_bin(length):
    return "short" if length <= SPMV_SHORT else ("medium" if length <= SPMV_SEG else "long")


def spg_class_of(bound):
    if bound <= 0:
        return SPG_CLS_EMPTY
    if bound <= SPG_TINY:
        return 0
    for c in range(SPG_LOGT_MAX - SPG_LOGT_MIN + 1):
        if bound <= (64 << c):
            return 1 + c
    return SPG_CLS_GLOBAL


def spg_lanes(cls):
    """lanes of the workgroup (team, for the tiny class) that takes a row of this class = segments per batch of spg_for_terms"""
    if cls == 0:
        return SPG_TINY_TEAM
    if cls == SPG_CLS_EMPTY:
        return 0
    if cls == SPG_CLS_GLOBAL:
        return 256
    return 64 if SPG_LOGT_MIN - 1 + cls <= 10 else 256


def spg_paths(bounds):
    """(rows_tiny, rows_hash, rows_global) of stats() for rows of these bounds"""
    cls = [spg_class_of(int(b)) for b in bounds]
    return (sum(c == 0 for c in cls), sum(1 <= c < SPG_CLS_GLOBAL for c in cls), sum(c == SPG_CLS_GLOBAL for c in cls))


def hash_home(col, logt):
    if isinstance(col, (int, np.integer)):
        return ((int(col) * 2654435761) & 0xFFFFFFFF) >> (32 - logt)
    c = np.asarray(col, dtype=np.uint64)
    return (((c * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - logt)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _colliding(logt, count, m):
    found, have, step = [], 0, 1 << 22
    for lo in range(0, m, step):
        c = np.arange(lo, min(m, lo + step), dtype=np.int64)
        hit = c[hash_home(c, logt) == (1 << logt) - 1]
        found.append(hit)
        have += len(hit)
        if have >= count:
            break
    return np.concatenate(found)[:count] if found else np.zeros(0, np.int64)


def colliding_columns(logt, count, m):
    """the first `count` columns below m whose home slot in a table of 2^logt slots is the last one (fewer when m is too small: the
    host test is where that fails)"""
    return _colliding(logt, count, m).copy()


# ---- designed products --------------------------------------------------------------------------------------------------------
def target_residue(p, sign=1):
    """the residue every designed product is congruent to.  p < 2^16: p//2 - 512 -- zp_small_lazy may be off by up to 256 before
    its final fix-up, so 512 below the half the lazy residue is the balanced one, its sign is fixed and a lane's i32 sum really
    reaches terms * (p//2 - 512).  Larger p: p//2 - 1 (the i64 lazy term is the balanced residue up to one p near the half)."""
    if p < 2**16:
        assert p // 2 > 1024, "a designed prime below 2^16 leaves room for the 512"
        t = p // 2 - 512
    else:
        t = p // 2 - 1
    return sign * t


def lift(x, p, rng, fraction):
    """x with about `fraction` of its entries replaced by x + s p, s != 0, inside int32 (left alone where no such s exists)"""
    x = np.asarray(x, dtype=np.int64).copy()
    pick = np.flatnonzero(rng.random(len(x)) < fraction)
    smin = -((x[pick] - INT32_MIN) // p)
    smax = (INT32_MAX - x[pick]) // p
    s = rng.integers(smin, smax + 1)
    s = np.where(s == 0, np.where(smax > 0, smax, smin), s)
    x[pick] += s * p
    return x


def inverse_times(t, a, p):
    """t / a mod p for every a (Python integers), balanced"""
    return bal(np.array([t * pow(int(u), -1, p) % p for u in np.asarray(a).reshape(-1)], dtype=np.int64), p)


def designed_pairs(p, count, rng, sign=1, unreduced=0.0):
    """a: random balanced non-zero values; x = t / a mod p, balanced, t = target_residue(p, sign); a fraction `unreduced` of the x
    lifted to unreduced int32"""
    a = rand_values(p, count, rng)
    x = inverse_times(target_residue(p, sign), a, p)
    if unreduced:
        x = lift(x, p, rng, unreduced)
    return a, x


# ---- CSR builders -------------------------------------------------------------------------------------------------------------
def rows_of_lengths(lengths, m, rng, values, cols_below=None):
    """a matrix whose row i has lengths[i] entries: columns distinct inside a row (below cols_below, default m), stored unsorted;
    values(count) gives the values of a row"""
    rows = []
    for l in lengths:
        rows.append((rng.permutation(cols_below or m)[:l], values(l)))
    return mat_from_rows(rows, m)


def host_transpose(M):
    row = np.repeat(np.arange(M.n), np.diff(M.ptr))
    order = np.argsort(M.j, kind="stable")
    ptr = np.zeros(M.m + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(np.bincount(M.j, minlength=M.m))
    return Mat(M.m, M.n, ptr, row[order], M.v[order])


# ---- exact references ------------------------------------------------------------------------------------------------------------
def ref_apply(ptr, j, v, X, Y, trans, p):
    """Y + op(A) X mod p as balanced int32, X (rows_in, k), Y (rows_out, k): every product reduced in uint64, then np.add.at
    (terms * p < 2^63); Python integers per output entry where that would not fit"""
    ptr = np.asarray(ptr, dtype=np.int64)
    j, v = np.asarray(j, dtype=np.int64), np.asarray(v, dtype=np.int64) % p
    row = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    src, dst = (row, j) if trans else (j, row)
    Xr = np.asarray(X, dtype=np.int64) % p
    acc = np.ascontiguousarray(np.asarray(Y, dtype=np.int64) % p)
    k = acc.shape[1]
    most = int(np.bincount(dst).max()) if len(dst) else 0
    if (most + 1) * p >= 2**63:
        big = acc.astype(object)
        for e in range(len(dst)):
            big[dst[e]] += (int(v[e]) * Xr[src[e]].astype(object)) % p
        acc = (big % p).astype(np.int64)
    else:
        flat = acc.reshape(-1)
        for c0 in range(0, k, 32):
            c1 = min(k, c0 + 32)
            prod = (v.astype(np.uint64)[:, None] * Xr[src, c0:c1].astype(np.uint64)) % np.uint64(p)  # < p^2 < 2^64
            idx = dst[:, None] * k + np.arange(c0, c1)[None, :]
            np.add.at(flat, idx.reshape(-1), prod.reshape(-1).astype(np.int64))
        acc %= p
    return np.where(2 * acc > p, acc - p, acc).astype(np.int32)


def canon(n, m, rows, cols, vals, p):
    """canonical CSR arrays (ptr, j, x) of the matrix sum of the terms (rows, cols, vals), vals in [0, p); also the number of
    distinct keys"""
    width = max(m, 1)
    key = rows.astype(np.int64) * width + cols.astype(np.int64)
    uk, inv, counts = np.unique(key, return_inverse=True, return_counts=True)
    if len(uk) and int(counts.max()) * p >= 2**63:
        big = np.zeros(len(uk), dtype=object)
        for t in range(len(key)):
            big[inv[t]] += int(vals[t])
        acc = (big % p).astype(np.int64)
    else:
        acc = np.zeros(len(uk), dtype=np.int64)
        np.add.at(acc, inv, vals.astype(np.int64))
        acc %= p
    keep = acc != 0
    distinct = len(uk)
    uk, acc = uk[keep], acc[keep]
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(ptr, uk // width + 1, 1)
    return np.cumsum(ptr), (uk % width).astype(np.int32), np.where(2 * acc > p, acc - p, acc).astype(np.int32), distinct


def ref_mul(A, B, p):
    assert A.m == B.n
    row_a = np.repeat(np.arange(A.n), np.diff(A.ptr))
    cnt = np.diff(B.ptr)[A.j] if len(A.j) else np.zeros(0, np.int64)
    ia = np.repeat(np.arange(len(A.j)), cnt)
    ib = np.repeat(B.ptr[A.j] if len(A.j) else np.zeros(0, np.int64), cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    prod = ((A.v[ia] % p).astype(np.uint64) * (B.v[ib] % p).astype(np.uint64)) % np.uint64(p)
    return canon(A.n, B.m, row_a[ia], B.j[ib], prod, p)


def ref_lincomb(sa, A, sb, B, p):
    rows, cols, vals = [], [], []
    for s, M in ((sa, A), (sb, B)):
        if M is None:
            continue
        rows.append(np.repeat(np.arange(M.n), np.diff(M.ptr)))
        cols.append(M.j)
        vals.append((((M.v % p).astype(np.uint64) * np.uint64(s % p)) % np.uint64(p)).astype(np.int64))
    return canon(A.n, A.m, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), p)


def ref_submatrix(A, r0, r1, c0, c1, p):
    row = np.repeat(np.arange(A.n), np.diff(A.ptr))
    keep = (row >= r0) & (row < r1) & (A.j >= c0) & (A.j < c1)
    return canon(r1 - r0, c1 - c0, row[keep] - r0, A.j[keep] - c0, A.v[keep] % p, p)


def product_bounds(A, B):
    """bound of every row of A B: the sum of the lengths of the rows of B its entries name"""
    lb = np.diff(B.ptr)
    out = np.zeros(A.n, dtype=np.int64)
    np.add.at(out, np.repeat(np.arange(A.n), np.diff(A.ptr)), lb[A.j] if len(A.j) else np.zeros(0, np.int64))
    return out


# ---- SpMV: the designed inputs ---------------------------------------------------------------------------------------------------
def spmv_designed(p, rng):
    """the 13 x 32769 matrix with the row lengths SPMV_LENGTHS, random balanced non-zero values"""
    return rows_of_lengths(SPMV_LENGTHS, max(SPMV_LENGTHS), rng, lambda l: rand_values(p, l, rng))


def spmv_short_plus_one(p, rng):
    """rows of every length 0 .. 32 and one medium row of 40 entries in the middle: short_all false, lists of a few rows"""
    lengths = list(range(0, 17)) + [40] + list(range(17, 33))
    return rows_of_lengths(lengths, 48, rng, lambda l: rand_values(p, l, rng))


# medium: a lane of the KW = 64 kernel takes it whole; long: three full segments and one entry; long: five and one -- 81921 terms,
# more than the 66591 of p//2 - 512 an i32 holds for p = 65521, so that the cut into segments is what keeps a lane's sum exact
LANE_ROWS = [SPMV_SEG, 3 * SPMV_SEG + 1, 5 * SPMV_SEG + 1]


def lane_worst_case(p, rng, sign=1):
    """(W, x, sums): W is 3 x 81921 with the row lengths LANE_ROWS, x the designed vector; every product W[i, c] x[c] is congruent to
    t = target_residue(p, sign), except the last stored entry of each full segment of a long row, chosen so that the segment's own
    sum is congruent to t: the partials k_spmv_combine adds are all t.  Segment s of a long row holds exactly the columns
    [s SEG, (s + 1) SEG), shuffled, so the segments are the same sets whether the entries come in stored order or by column (the
    order a transpose of the transpose gives them).  sums[i] is an integer congruent to row i of W x."""
    t = target_residue(p, sign)
    m = LANE_ROWS[-1]
    a, x = designed_pairs(p, m, rng, sign)
    mid_cols = rng.permutation(m)[: LANE_ROWS[0]]
    rows, sums = [(mid_cols, a[mid_cols])], [LANE_ROWS[0] * t]
    for length in LANE_ROWS[1:]:
        full = length // SPMV_SEG
        cols_all, vals_all = [], []
        for s in range(full):
            cols = s * SPMV_SEG + rng.permutation(SPMV_SEG)
            vals = a[cols].copy()
            vals[-1] = inverse_times((t - (SPMV_SEG - 1) * t) % p, x[cols[-1:]], p)[0]
            cols_all.append(cols)
            vals_all.append(vals)
        cols_all.append(np.array([full * SPMV_SEG]))
        vals_all.append(a[full * SPMV_SEG: full * SPMV_SEG + 1])
        rows.append((np.concatenate(cols_all), np.concatenate(vals_all)))
        sums.append((full + 1) * t)
    return mat_from_rows(rows, m), x, sums


BINNED_STORED = [SPMV_SHORT + 1, SPMV_SEG + 1, 2 * SPMV_SEG + 1]


def binned_longer(p, rng):
    """rows of 33, 16385 and 32769 stored entries, all multiples of p except 5 (the first, the last and three between), the
    survivors unreduced where int32 has room: the rows are binned medium, long, long by their stored lengths and hold 5 entries on
    the device, so the later segments of the long rows start past the end of the row"""
    m = BINNED_STORED[-1]
    rows = []
    for l in BINNED_STORED:
        cols = rng.permutation(m)[:l]
        vals = lift(np.zeros(l, dtype=np.int64), p, rng, 0.7)  # multiples of p, many of them not 0
        live = np.array([0, l // 3, l // 2, l - 2, l - 1])
        vals[live] = lift(rand_values(p, 5, rng), p, rng, 1.0)
        rows.append((cols, vals))
    return mat_from_rows(rows, m)


# ---- sparse algebra: rows on the class edges ---------------------------------------------------------------------------------------
def class_edge_product(E, p, rng, pad):
    """(A, B, bounds): C = A B has rows of bound E and E + 1
      rows 0, 1   all columns distinct, stored unsorted, from two and three rows of B
      rows 2, 3   E and E + 1 designed products (each congruent to t) on one column
      rows 4, 5   the same with a last product chosen so that the sum is 0 mod p: the row comes out empty
      row 6       E designed products congruent to -t on one column
    and, with pad, enough rows of one entry (bound 1) that nnz(A) <= 8 n: k_spg_size sizes the rows, k_spg_size_wave otherwise"""
    m = SPG_M
    t = target_residue(p)
    perm = rng.permutation(m)
    d1, d2, d3 = perm[: E // 2], perm[E // 2: E], perm[E: E + 1]
    star = int(perm[E + 1])
    a, x = designed_pairs(p, E + 1, rng)
    brows = [(d, rand_values(p, len(d), rng)) for d in (d1, d2, d3)] + [(np.array([star]), x[k: k + 1]) for k in range(E + 1)]
    B = mat_from_rows(brows, m)

    def on_star(count, last=None, sign=1):
        order = rng.permutation(count)
        vals = sign * a[order]
        if last is not None:  # the last stored product makes the sum `last` mod p
            vals[-1] = inverse_times((last - (count - 1) * sign * t) % p, x[order[-1:]], p)[0]
        return 3 + order, vals

    arows = [(np.array([0, 1]), rand_values(p, 2, rng)), (np.array([1, 2, 0]), rand_values(p, 3, rng)),
             on_star(E), on_star(E + 1), on_star(E, last=0), on_star(E + 1, last=0), on_star(E, sign=-1)]
    bounds = [E, E + 1, E, E + 1, E, E + 1, E]
    if pad:
        nnz = sum(len(c) for c, _ in arows)
        extra = max(0, -(-(nnz - 8 * len(arows)) // 7))
        arows += [(np.array([2]), rand_values(p, 1, rng)) for _ in range(extra)]
        bounds += [1] * extra
    return mat_from_rows(arows, B.n), B, bounds


LINCOMB_SCALARS = (2**32 + 12345, -(2**40) - 7)


def class_edge_lincomb(E, p, rng):
    """(A, B, sa, sb, bounds): len(A row) + len(B row) is E and E + 1 in three shapes: disjoint columns; E // 4 shared columns on
    which sa A + sb B cancels; one operand's row empty"""
    m = SPG_M
    sa, sb = LINCOMB_SCALARS
    h, q = E // 2, E // 4
    arows, brows, bounds = [], [], []
    for extra in (0, 1):
        perm = rng.permutation(m)
        arows.append((perm[:h], rand_values(p, h, rng)))                               # disjoint
        brows.append((perm[h: E + extra], rand_values(p, E + extra - h, rng)))
        perm = rng.permutation(m)
        av = rand_values(p, h, rng)
        lb = E + extra - h
        bcols = np.concatenate([perm[:q][::-1], perm[h: h + lb - q]])                    # the first q columns of A's row, reversed
        bv = rand_values(p, lb, rng)
        bv[:q] = bal(np.array([(-sa * int(u) * pow(sb, -1, p)) % p for u in av[:q][::-1]], dtype=np.int64), p)
        mix = rng.permutation(lb)
        arows.append((perm[:h], av))                                                    # overlapping, cancelling on the overlap
        brows.append((bcols[mix], bv[mix]))
        perm = rng.permutation(m)
        one = (perm[: E + extra], rand_values(p, E + extra, rng))                       # one operand empty
        none = (np.zeros(0, np.int64), np.zeros(0, np.int64))
        arows.append(one if extra == 0 else none)
        brows.append(none if extra == 0 else one)
        bounds += [E + extra] * 3
    return mat_from_rows(arows, m), mat_from_rows(brows, m), sa, sb, bounds


SUBMATRIX_FREE = 8000  # no stored column at or above it: the window [8000, 8100) keeps nothing


def class_edge_submatrix(E, p, rng):
    """(A, windows, bounds): rows of E and E + 1 stored entries (the bound of a submatrix row is its stored length, whatever the
    window keeps), columns below 8000 of 8192"""
    lengths = [E, E + 1, 0, E + 1, E]
    A = rows_of_lengths(lengths, SPG_M, rng, lambda l: rand_values(p, l, rng), cols_below=SUBMATRIX_FREE)
    windows = [(0, SPG_M), (1000, 3048), (SUBMATRIX_FREE, SUBMATRIX_FREE + 100), (0, 1), (SUBMATRIX_FREE - 1, SUBMATRIX_FREE + 1)]
    return A, windows, lengths


# ---- sparse algebra: segment batches -------------------------------------------------------------------------------------------------
SEG_B_ROWS, SEG_B_COLS, SEG_B_LONG = 400, 40, 40


def _seg_plan():
    """(lanes, segment lengths) of every row of A: the length of the row of B each stored entry names, laid out against the batch
    size BS = lanes of the class the row's bound falls in.  E = empty rows of B first / last in a batch, in runs across a batch
    edge, as one whole batch."""
    plans = []

    def plan(lanes, L, fill, empty):
        seg = [fill(i) for i in range(L)]
        for i in empty:
            if 0 <= i < L:
                seg[i] = 0
        plans.append((lanes, seg))

    three = lambda i: 3
    cyc = lambda i: 1 + i % 3
    # 63, 64, 65 entries: 64-lane classes
    plan(64, 63, cyc, [0, 62])                                     # first and last of a batch that is not full
    plan(64, 64, cyc, [0, 63])                                     # first and last of a full batch
    plan(64, 65, cyc, [61, 62, 63, 64])                            # a run across the edge; the second batch is one empty segment
    # 255, 256, 257 entries at most 1 long: still 64 lanes (bound <= 512), four or five batches
    plan(64, 255, lambda i: 1, list(range(64, 128)) + [0, 128, 191, 192, 254])       # the second batch is empty
    plan(64, 256, lambda i: 1, list(range(125, 131)) + [63, 64, 255])                # a run across the edge of batches 1 | 2
    plan(64, 257, lambda i: 1, list(range(192, 257)))                                # the last two batches are empty
    # the same lengths of A's row with rows of B of 3: 256 lanes (bound > 512), one or two batches
    plan(256, 255, three, [0, 254])
    plan(256, 256, three, [0, 255])
    plan(256, 257, three, [254, 255, 256])
    # 513 and 1025 entries
    plan(64, 513, lambda i: 1, [i for i in range(513) if (i // 64) % 2 == 1])         # every other batch of nine is empty
    plan(256, 513, three, list(range(256, 512)))                                     # the middle batch is empty, then one segment
    plan(256, 1025, lambda i: i % 4, list(range(512, 768)) + list(range(253, 260)) + [1024])
    # 2049 entries of 3: the global class, nine batches of 256
    plan(256, 2049, three, list(range(256, 512)) + [0, 255, 512, 2048])
    # every segment empty: bound 0, no class; and a single non-empty segment, the last one
    plan(0, 100, lambda i: 0, [])
    plan(SPG_TINY_TEAM, 130, lambda i: 0, [])
    plans[-1][1][-1] = 3
    plan(64, 130, lambda i: 0, [])
    plans[-1][1][-1] = SEG_B_LONG
    return plans


def segment_batch_case(p, rng):
    """(A, B, lanes, bounds): B has rows of 0, 1, 2, 3 entries (row r: r % 4) on 40 columns, so that sums collide and, for p = 3,
    cancel, and one last row of 40 entries; the rows of A follow _seg_plan"""
    brows = []
    for r in range(SEG_B_ROWS):
        brows.append((rng.permutation(SEG_B_COLS)[: r % 4], rand_values(p, r % 4, rng)))
    brows.append((rng.permutation(SEG_B_COLS)[:SEG_B_LONG], rand_values(p, SEG_B_LONG, rng)))
    B = mat_from_rows(brows, SEG_B_COLS)
    arows, lanes, bounds = [], [], []
    for ln, seg in _seg_plan():
        seg = np.array(seg)
        cols = np.where(seg == SEG_B_LONG, SEG_B_ROWS, 4 * rng.integers(0, SEG_B_ROWS // 4, size=len(seg)) + np.minimum(seg, 3))
        arows.append((cols, rand_values(p, len(seg), rng)))
        lanes.append(ln)
        bounds.append(int(seg.sum()))
    return mat_from_rows(arows, B.n), B, lanes, bounds


# ---- sparse algebra: probe chains ---------------------------------------------------------------------------------------------------
PROBE_M = {7: 1 << 14, 13: 1 << 26}


def probe_chain_case(logt, p, rng):
    """(A, B, bounds): every row of C = A B has bound 2^(logt - 1), the most its class allows, on columns whose home is the last slot
    of the table: the chain wraps to slot 0 and runs on
      row 0   2^(logt - 1) distinct columns, descending: the table is at its full permitted load, the chain is LIST slots long
      row 1   half as many columns, met twice, the second time in reverse order (`old == c` at the end of a long probe)
      row 2   a quarter as many, four times, in four orders"""
    m = PROBE_M[logt]
    half = 1 << (logt - 1)
    cols = colliding_columns(logt, half, m)
    brows = [(cols[::-1], rand_values(p, half, rng)),
             (cols[: half // 2], rand_values(p, half // 2, rng)), (cols[: half // 2][::-1], rand_values(p, half // 2, rng))]
    for _ in range(4):
        brows.append((rng.permutation(cols[half // 2: half // 2 + half // 4]), rand_values(p, half // 4, rng)))
    B = mat_from_rows(brows, m)
    A = mat_from_rows([(np.array([0]), rand_values(p, 1, rng)), (np.array([1, 2]), rand_values(p, 2, rng)),
                       (np.array([3, 4, 5, 6]), rand_values(p, 4, rng))], B.n)
    return A, B, [half, half, half]


# ---- sparse algebra: tiny rows at capacity ------------------------------------------------------------------------------------------
TINY_ROWS = 37  # two workgroups of 16 teams and one with 5 busy teams, 11 idle


def tiny_capacity_case(p, rng):
    """(A, B, bounds): 37 rows of C = A B of bound exactly 32, cycling through: 32 designed products on one column; the same with a
    last product that makes the sum 0; 32 distinct columns stored descending; 16 + 16 from two segments with 8 shared columns"""
    m = 100
    t = target_residue(p)
    a, x = designed_pairs(p, SPG_TINY, rng)
    star = 77
    desc = np.sort(rng.permutation(m)[:SPG_TINY])[::-1]
    perm = rng.permutation(m)
    brows = [(np.array([star]), x[k: k + 1]) for k in range(SPG_TINY)]
    brows += [(desc, rand_values(p, SPG_TINY, rng)), (perm[:16], rand_values(p, 16, rng)), (perm[8:24][::-1], rand_values(p, 16, rng))]
    B = mat_from_rows(brows, m)
    arows = []
    for i in range(TINY_ROWS):
        kind = i % 4
        if kind in (0, 1):
            order = rng.permutation(SPG_TINY)
            vals = a[order].copy()
            if kind == 1:
                vals[-1] = inverse_times((-(SPG_TINY - 1) * t) % p, x[order[-1:]], p)[0]
            arows.append((order, vals))
        elif kind == 2:
            arows.append((np.array([SPG_TINY]), rand_values(p, 1, rng)))
        else:
            arows.append((np.array([SPG_TINY + 1, SPG_TINY + 2]), rand_values(p, 2, rng)))
    return mat_from_rows(arows, B.n), B, [SPG_TINY] * TINY_ROWS


TINY_WINDOW = (100, 200)


def tiny_capacity_submatrix(p, rng):
    """(A, window, bounds): 37 rows of 32 stored entries whose stored order alternates a column inside the window [100, 200) and one
    outside it (below or above); every fifth row lies entirely outside"""
    m, (c0, c1) = 300, TINY_WINDOW
    rows = []
    for i in range(TINY_ROWS):
        inside = c0 + rng.permutation(c1 - c0)[:16]
        outside = np.concatenate([np.arange(c0), np.arange(c1, m)])[rng.permutation(m - (c1 - c0))[:32]]
        cols = outside.copy()
        if i % 5 != 4:
            cols[(i % 2)::2] = inside  # in, out, in, out .. or out, in, out, in ..
        rows.append((cols, rand_values(p, 32, rng)))
    return mat_from_rows(rows, m), TINY_WINDOW, [32] * TINY_ROWS
