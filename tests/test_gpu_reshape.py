"""Transpose, permutation and concatenation of resident matrices (spasm_amd_dcsr_transpose / _permute / _vcat / _hcat; DeviceCSR.T,
.permute, vcat, hcat).  Every expected matrix is built with numpy alone, on COO triples (row, column, value) or on dense images:
the operations move values and never compute one, so a result must agree with its reference byte for byte, and every download is
checked to be canonical (columns strictly ascending inside each row, no stored zero, nzmax == nnz == p[n])."""
import ctypes as C
import gc
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PRIMES = [127, 65521, 0xFFFFFFFB]
_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spasm.jl_amd", "csrc", "reshape.hpp")
with open(_SRC) as _fh:
    L = int(re.search(r"RSH_GROUP_MAX = (\d+)", _fh.read()).group(1))  # longest row the workgroup path orders


def csr_arrays(A):
    k = int(A.p[A.n])
    return np.asarray(A.p, dtype=np.int64).copy(), A.j[:k].astype(np.int64), A.x[:k].astype(np.int64)


def coo_of(A):
    ptr, j, x = csr_arrays(A)
    return np.repeat(np.arange(A.n, dtype=np.int64), np.diff(ptr)), j, x


def csr_of(n, m, r, c, v):
    """canonical CSR arrays of the triples (distinct positions, non-zero values)"""
    order = np.lexsort((c, r))
    r, c, v = np.asarray(r, dtype=np.int64)[order], np.asarray(c, dtype=np.int64)[order], np.asarray(v, dtype=np.int64)[order]
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(ptr, r + 1, 1)
    return np.cumsum(ptr), c.astype(np.int32), v.astype(np.int32)


def make(S, n, m, r, c, v, p):
    ptr, j, x = csr_of(n, m, r, c, v)
    return S.CSR.from_arrays(n, m, ptr, j, x, prime=p)


def rand_coo(n, m, density, p, rng, empty=False):
    """triples of an n x m matrix: balanced non-zero values, halfp and mhalfp among them; empty: every third row and every
    fourth column hold nothing"""
    mask = rng.random((n, m)) < density
    if empty:
        mask[::3, :] = False
        mask[:, ::4] = False
    r, c = np.nonzero(mask)
    h = p // 2  # halfp; mhalfp = -halfp for an odd prime
    v = rng.integers(1, p, size=len(r), dtype=np.int64)
    v = np.where(v > h, v - p, v)
    v[0::7] = h
    v[1::7] = -h
    return r.astype(np.int64), c.astype(np.int64), v


def rand_csr(S, n, m, density, p, rng, empty=False):
    return make(S, n, m, *rand_coo(n, m, density, p, rng, empty), p)


def dense_of(A):
    r, c, v = coo_of(A)
    M = np.zeros(A.shape, dtype=np.int64)
    M[r, c] = v
    return M


def csr_of_dense(M):
    r, c = np.nonzero(M)
    return csr_of(M.shape[0], M.shape[1], r, c, M[r, c])


def check_canonical(Cm):
    ptr, j, x = csr_arrays(Cm)
    k = int(ptr[-1])
    assert ptr[0] == 0 and np.all(np.diff(ptr) >= 0)
    assert Cm.nzmax == k, (Cm.nzmax, k)
    if k:
        inner = np.ones(k, dtype=bool)
        inner[ptr[:-1][np.diff(ptr) > 0]] = False  # the first entry of each row
        assert np.all(np.diff(j)[inner[1:]] > 0), "columns must strictly ascend inside every row"
        assert j.min() >= 0 and j.max() < Cm.m and np.all(x != 0)


def same(d, shape, want, what=""):
    """the resident matrix d downloads to exactly the arrays want = (p, j, x), in canonical form"""
    ptr, j, x = want
    Cm = d.download()
    assert d.shape == tuple(shape) == Cm.shape, (what, d.shape, shape)
    check_canonical(Cm)
    k = int(ptr[-1])
    assert d.nnz == k == int(Cm.p[Cm.n]), (what, d.nnz, k)
    assert np.array_equal(np.asarray(Cm.p), ptr), what
    assert np.array_equal(Cm.j[:k], j) and np.array_equal(Cm.x[:k], x), what


def ref_transpose(A):
    r, c, v = coo_of(A)
    return csr_of(A.m, A.n, c, r, v)


def ref_permute(A, p=None, q=None):
    """numpy's A[np.ix_(p, q)] on triples: old row p[i] becomes row i, old column q[k] becomes column k"""
    r, c, v = coo_of(A)
    if p is not None:
        pinv = np.empty(A.n, dtype=np.int64)
        pinv[np.asarray(p)] = np.arange(A.n)
        r = pinv[r]
    if q is not None:
        qinv = np.empty(A.m, dtype=np.int64)
        qinv[np.asarray(q)] = np.arange(A.m)
        c = qinv[c]
    return csr_of(A.n, A.m, r, c, v)


SHAPES = [(0, 0), (0, 5), (5, 0), (1, 1), (7, 5), (300, 200)]


@pytest.mark.parametrize("p", PRIMES)
def test_transpose_entry_for_entry(S, p):
    rng = np.random.default_rng(p % 1009)
    for (n, m) in SHAPES:
        A = rand_csr(S, n, m, 1.0 if n * m == 1 else (0.4 if n * m < 100 else 0.05), p, rng)
        with S.DeviceCSR(A) as d:
            t = d.T
            assert t.prime == p
            same(t, (m, n), ref_transpose(A), (p, n, m))
            assert np.array_equal(dense_of(t.download()), dense_of(A).T)
            assert t.T.equals(d) and d.transpose().equals(t)
            st = t.stats()
            assert st["op"] == 4 and st["flops"] == st["entries"] == t.nnz and st["chunks"] == 1
    # empty rows and empty columns; the extreme values are present
    A = rand_csr(S, 61, 47, 0.2, p, rng, empty=True)
    _, _, x = csr_arrays(A)
    assert x.max() == p // 2 and x.min() == -(p // 2)
    with S.DeviceCSR(A) as d:
        same(d.T, (47, 61), ref_transpose(A))
        assert d.T.T.equals(d)
    # (A B)^T = B^T A^T on the device
    A = rand_csr(S, 300, 200, 0.05, p, rng)
    B = rand_csr(S, 200, 150, 0.05, p, rng)
    with S.DeviceCSR(A) as a, S.DeviceCSR(B) as b:
        left, right = (a @ b).T, b.T @ a.T
        assert left.shape == (150, 300) and left.nnz > 0 and left.equals(right)


def paths_matrix(S, p):
    """(2 L + 5) x 12 whose columns hold 1, 63, 64, 65, L, L + 1 entries, three full columns over the first 2 L rows, 500, 2000
    entries, and nothing: the rows of its transpose fall into every class of the ordering step"""
    rng = np.random.default_rng(31)
    n = 2 * L + 5
    counts = [1, 63, 64, 65, L, L + 1, 2 * L, 2 * L, 2 * L, 500, 2000, 0]
    r = np.concatenate([np.arange(2 * L) if k == 2 * L else np.sort(rng.permutation(n)[:k]) for k in counts]).astype(np.int64)
    c = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    v = rng.integers(1, p, size=len(r), dtype=np.int64)
    v = np.where(v > p // 2, v - p, v)
    return make(S, n, len(counts), r, c, v, p), counts


@pytest.mark.parametrize("p", [65521, 0xFFFFFFFB])
def test_every_ordering_path_is_taken(S, p):
    A, counts = paths_matrix(S, p)
    want_t = ref_transpose(A)
    with S.DeviceCSR(A) as d:
        t = d.T
        st = t.stats()
        print("transpose stats", p, st)
        assert st["rows_tiny"] == 2 and st["rows_hash"] == 4 and st["rows_global"] == 4, st  # 63 64 | 65 500 2000 L | L + 1 and 3 x 2 L
        assert st["max_bound"] == 2 * L and st["entries"] == sum(counts)
        same(t, (len(counts), A.n), want_t)
    # the same rows under a permutation of their columns
    T = S.CSR.from_arrays(len(counts), A.n, *want_t, prime=p)
    rng = np.random.default_rng(32)
    q = rng.permutation(T.m)
    with S.DeviceCSR(T) as d:
        e = d.permute(q=q)
        st = e.stats()
        print("permute stats", p, st)
        assert st["op"] == 5 and st["rows_tiny"] > 0 and st["rows_hash"] > 0 and st["rows_global"] > 0, st
        same(e, T.shape, ref_permute(T, None, q))


def test_permute(S):
    p = 65521
    rng = np.random.default_rng(33)
    n, m = 257, 193
    A = rand_csr(S, n, m, 0.08, p, rng)
    M = dense_of(A)
    P, Q = rng.permutation(n), rng.permutation(m)
    with S.DeviceCSR(A) as d:
        both = d.permute(P, Q)
        same(both, (n, m), ref_permute(A, P, Q))
        assert np.array_equal(dense_of(both.download()), M[np.ix_(P, Q)])
        rows = d.permute(P)
        same(rows, (n, m), ref_permute(A, P, None))
        st = rows.stats()
        assert st["rows_tiny"] == st["rows_hash"] == st["rows_global"] == 0 and st["op"] == 5, st
        cols = d.permute(q=Q)
        same(cols, (n, m), ref_permute(A, None, Q))
        assert np.array_equal(dense_of(cols.download()), M[:, Q])
        assert cols.stats()["rows_tiny"] > 0
        # qinv given directly: an entry on column j lands on column qinv[j]
        qinv = np.empty(m, dtype=np.int64)
        qinv[Q] = np.arange(m)
        assert d.permute(qinv=qinv).equals(cols) and d.permute(P, qinv=qinv).equals(both)
        ident = d.permute()
        same(ident, (n, m), csr_arrays(A))
        assert ident.equals(d) and d.permute(np.arange(n), np.arange(m)).equals(d)
        # and back
        pinv = np.empty(n, dtype=np.int64)
        pinv[P] = np.arange(n)
        assert both.permute(pinv, qinv).equals(d)
        # the C entry refuses what is not a permutation, with a text, and leaves the operand as it was
        lib = S._abi.lib()
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
        rep, out = P.copy(), P.copy()
        rep[5] = rep[6]
        out[0] = n
        neg = Q.copy()
        neg[m - 1] = -1
        for (pp, qq, word) in ((rep, None, "repeated"), (out, None, "out of range"), (None, neg, "out of range"), (P, np.zeros(m), "repeated")):
            h = lib.spasm_amd_dcsr_permute(d._h, None if pp is None else i32(pp), None if qq is None else i32(qq))
            assert not h and "permutation" in S._abi.last_error() and word in S._abi.last_error(), S._abi.last_error()
        same(d, (n, m), csr_arrays(A))
        d.permute(P)
        assert S._abi.last_error() == ""


def test_vcat_and_hcat(S):
    p = 0xFFFFFFFB
    rng = np.random.default_rng(34)
    tall = [rand_csr(S, k, 23, 0.2, p, rng, empty=(k == 40)) for k in (17, 0, 40, 1, 0)]     # equal columns; operands without rows
    wide = [rand_csr(S, 31, k, 0.2, p, rng, empty=(k == 40)) for k in (0, 19, 40, 0, 3)]     # equal rows; operands without columns
    with S.DeviceCSR(tall[0]) as t0, S.DeviceCSR(tall[1]) as t1, S.DeviceCSR(tall[2]) as t2, S.DeviceCSR(tall[3]) as t3, S.DeviceCSR(tall[4]) as t4:
        ds = [t0, t1, t2, t3, t4]
        for pick in ([0], [1], [0, 2], [1, 0], [0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 2]):
            M = np.vstack([dense_of(tall[k]) for k in pick])
            v = S.vcat(*[ds[k] for k in pick])
            same(v, M.shape, csr_of_dense(M), ("vcat", pick))
            st = v.stats()
            assert st["op"] == 6 and st["rows_tiny"] == st["rows_hash"] == st["rows_global"] == 0 and st["entries"] == v.nnz
            assert ds[pick[0]].vcat(*[ds[k] for k in pick[1:]]).equals(v)
    with S.DeviceCSR(wide[0]) as w0, S.DeviceCSR(wide[1]) as w1, S.DeviceCSR(wide[2]) as w2, S.DeviceCSR(wide[3]) as w3, S.DeviceCSR(wide[4]) as w4:
        ds = [w0, w1, w2, w3, w4]
        for pick in ([1], [0], [1, 2], [0, 1], [0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 2]):
            M = np.hstack([dense_of(wide[k]) for k in pick])
            h = S.hcat(*[ds[k] for k in pick])
            same(h, M.shape, csr_of_dense(M), ("hcat", pick))
            st = h.stats()
            assert st["op"] == 7 and st["rows_tiny"] == st["rows_hash"] == st["rows_global"] == 0 and st["entries"] == h.nnz
            assert ds[pick[0]].hcat(*[ds[k] for k in pick[1:]]).equals(h)
    # long rows go through the wave-per-row copy
    A = rand_csr(S, 20, 900, 0.5, p, rng)
    B = rand_csr(S, 20, 700, 0.5, p, rng)
    with S.DeviceCSR(A) as a, S.DeviceCSR(B) as b:
        M = np.hstack([dense_of(A), dense_of(B)])
        same(S.hcat(a, b), M.shape, csr_of_dense(M))
        # vcat(A^T, B^T)^T = hcat(A, B)
        assert S.vcat(a.T, b.T).T.equals(S.hcat(a, b))
        assert S.vcat(a.T, b.T).equals(S.hcat(a, b).T)
        # the C entry refuses shapes and primes that differ, with a text
        lib = S._abi.lib()
        Cp = rand_csr(S, 20, 900, 0.1, 127, rng)
        with S.DeviceCSR(Cp) as c, a.T as at:
            arr = lambda *hs: (C.c_void_p * len(hs))(*hs)
            assert not lib.spasm_amd_dcsr_vcat(2, arr(a._h, b._h)) and "dimension" in S._abi.last_error()
            assert not lib.spasm_amd_dcsr_hcat(2, arr(a._h, at._h)) and "dimension" in S._abi.last_error()
            assert not lib.spasm_amd_dcsr_vcat(2, arr(a._h, c._h)) and "prime" in S._abi.last_error()
            assert not lib.spasm_amd_dcsr_hcat(2, arr(c._h, a._h)) and "prime" in S._abi.last_error()
            assert not lib.spasm_amd_dcsr_hcat(2, arr(a._h, None)) and "NULL" in S._abi.last_error()
            assert not lib.spasm_amd_dcsr_vcat(0, arr(a._h)) and "at least one" in S._abi.last_error()
            assert not lib.spasm_amd_dcsr_vcat(1, None) and S._abi.last_error() != ""
            assert not lib.spasm_amd_dcsr_transpose(None) and "NULL" in S._abi.last_error()
        same(a, A.shape, csr_arrays(A))
        same(b, B.shape, csr_arrays(B))


def raw(Cm):
    k = int(Cm.p[Cm.n])
    return np.asarray(Cm.p).tobytes(), Cm.j[:k].tobytes(), Cm.x[:k].tobytes()


def test_canonical_and_deterministic(S):
    p = 65521
    A, _ = paths_matrix(S, p)
    rng = np.random.default_rng(35)
    B = rand_csr(S, A.n, 7, 0.01, p, rng)
    P, Q = rng.permutation(A.n), rng.permutation(A.m)
    with S.DeviceCSR(A) as a, S.DeviceCSR(B) as b, a.T as at:
        P2 = rng.permutation(at.shape[1])
        ops = {
            "transpose": lambda: a.T,
            "permute": lambda: a.permute(P, Q),
            "permute long rows": lambda: at.permute(q=P2),
            "vcat": lambda: S.vcat(a, a),
            "hcat": lambda: S.hcat(a, b, a),
        }
        for name, op in ops.items():
            outs = []
            for _ in range(3):
                Cm = op().download()
                check_canonical(Cm)
                outs.append(raw(Cm))
            assert outs[0] == outs[1] == outs[2], name


def test_non_canonical_upload(S):
    """unsorted rows, duplicate columns (some summing to zero mod p), explicit zeros: every operation sees the canonical form"""
    p = 127
    rng = np.random.default_rng(36)
    n, m = 90, 70
    r, c, v = rand_coo(n, m, 0.15, p, rng)
    extra = rng.integers(0, len(r), size=60)
    r2 = np.concatenate([r, r[extra[:30]], r[extra[:30]], r[extra[30:]], rng.integers(0, n, size=20)])
    c2 = np.concatenate([c, c[extra[:30]], c[extra[:30]], c[extra[30:]], rng.integers(0, m, size=20)])
    v2 = np.concatenate([v, rng.integers(1, p, size=30), np.zeros(30, np.int64), -v[extra[30:]], np.zeros(20, np.int64)])
    v2[len(r) + 30:len(r) + 60] = -(v2[len(r):len(r) + 30])  # a pair that cancels on top of the entry that stays
    order = rng.permutation(len(r2))  # then grouped by row only: the columns inside a row stay shuffled
    order = order[np.argsort(r2[order], kind="stable")]
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(ptr, r2 + 1, 1)
    messy = S.CSR.from_arrays(n, m, np.cumsum(ptr), c2[order].astype(np.int32), v2[order].astype(np.int32), prime=p)
    with S.DeviceCSR(messy) as d:
        canon = d.lincomb(1)
        assert canon.nnz < messy.nzmax and canon.equals(d)
        K = canon.download()
        check_canonical(K)
        P, Q = rng.permutation(n), rng.permutation(m)
        same(d.T, (m, n), ref_transpose(K))
        same(d.permute(P, Q), (n, m), ref_permute(K, P, Q))
        same(d.permute(P), (n, m), ref_permute(K, P, None))
        Mk = dense_of(K)
        same(S.vcat(d, canon, d), (3 * n, m), csr_of_dense(np.vstack([Mk, Mk, Mk])))
        same(S.hcat(d, d), (n, 2 * m), csr_of_dense(np.hstack([Mk, Mk])))
        assert d.T.equals(canon.T) and S.hcat(canon, d).equals(S.hcat(d, canon))
        # the upload itself is left as it was (its values are held as balanced residues)
        U = d.download()
        k = int(messy.p[n])
        assert np.array_equal(np.asarray(U.p), np.asarray(messy.p)) and np.array_equal(U.j[:k], messy.j[:k])
        assert np.all((U.x[:k].astype(np.int64) - messy.x[:k].astype(np.int64)) % p == 0)


def components_matrix(S, p, rng, nblocks=40):
    """a matrix of nblocks connected components (each a small dense-ish square block), its rows and columns shuffled"""
    sizes = rng.integers(2, 7, size=nblocks)
    n = int(sizes.sum())
    r, c, v = [], [], []
    at = 0
    for s in sizes:
        blk = rng.integers(1, p, size=(s, s))
        blk[rng.random((s, s)) < 0.3] = 0
        blk[np.arange(s), np.arange(s)] = rng.integers(1, p, size=s)  # connected through the first row and the diagonal
        blk[0, :] = rng.integers(1, p, size=s)
        rr, cc = np.nonzero(blk)
        r.append(rr + at)
        c.append(cc + at)
        v.append(blk[rr, cc])
        at += s
    r, c, v = np.concatenate(r), np.concatenate(c), np.concatenate(v).astype(np.int64)
    v = np.where(v > p // 2, v - p, v)
    pr, pc = rng.permutation(n), rng.permutation(n)
    return make(S, n, n, pr[r], pc[c], v, p), nblocks


def test_block_diagonal_form_with_the_blocks(S):
    p = 65521
    rng = np.random.default_rng(37)
    A, nblocks = components_matrix(S, p, rng)
    with S.DeviceCSR(A) as d, S.DeviceBlocks(d) as blocks:
        assert len(blocks) == nblocks
        mp = blocks.maps()
        e = d.permute(mp["block_rows"], mp["block_cols"])
        assert e.stats()["rows_tiny"] > 0
        E = e.download()
        check_canonical(E)
        r, c, _ = coo_of(E)
        rs, cs = mp["row_start"], mp["col_start"]
        rb = np.searchsorted(rs, r, side="right") - 1
        cb = np.searchsorted(cs, c, side="right") - 1
        assert np.array_equal(rb, cb), "an entry lies outside the diagonal windows"
        for b in range(nblocks):
            W = e[int(rs[b]):int(rs[b + 1]), int(cs[b]):int(cs[b + 1])].download()
            Bk = blocks.fetch(b)
            assert W.shape == Bk.shape and raw(W) == raw(Bk), b


def test_right_sided_solve_through_the_transpose(S):
    """BatchSolver solves X A' = B; with A' = A^T that is A x = b for every row b of B"""
    p = 65521
    rng = np.random.default_rng(38)
    n = 12
    M = rng.integers(1, p, size=(n, n))
    M[rng.random((n, n)) < 0.4] = 0
    M[np.arange(n), np.arange(n)] = rng.integers(1, p, size=n)
    A = S.CSR.from_arrays(n, n, *csr_of_dense(np.where(M > p // 2, M - p, M)), prime=p)
    X0 = rng.integers(0, p, size=(5, n))
    Bd = np.array([[sum(int(M[i, k]) * int(X0[t, k]) for k in range(n)) % p for i in range(n)] for t in range(5)], dtype=np.int64)  # rows b = A x0
    B = S.CSR.from_arrays(5, n, *csr_of_dense(np.where(Bd > p // 2, Bd - p, Bd)), prime=p)
    with S.DeviceCSR(A) as d:
        At = d.T.download()
    with S.BatchSolver([At]) as solver:
        (X,), (ok,) = solver.solve([B])
    assert ok.all() and X.shape == (5, n)
    Xd = dense_of(X)
    for t in range(5):
        for i in range(n):
            lhs = sum(int(M[i, k]) * int(Xd[t, k]) for k in range(n))  # exact Python integers
            assert (lhs - int(Bd[t, i])) % p == 0, (t, i)


def test_lifetime(S):
    p = 127
    rng = np.random.default_rng(39)
    A = rand_csr(S, 50, 40, 0.1, p, rng)
    B = rand_csr(S, 50, 40, 0.1, p, rng)
    a, b = S.DeviceCSR(A), S.DeviceCSR(B)
    t, v, h, e = a.T, S.vcat(a, b), S.hcat(a, b), a.permute(np.arange(50)[::-1].copy())
    want_t, want_v = ref_transpose(A), csr_of_dense(np.vstack([dense_of(A), dense_of(B)]))
    a.close()
    b.close()
    del A, B
    gc.collect()
    same(t, (40, 50), want_t)  # a result does not depend on its operands
    same(v, (100, 40), want_v)
    # results as operands
    g = t @ h
    assert g.shape == (40, 80) and g.nnz > 0 and g.T.equals(h.T @ t.T)
    assert (e @ t).shape == (50, 50)
    for call in (lambda: a.T, lambda: a.permute(), lambda: S.vcat(t.T, a), lambda: S.hcat(a), lambda: b.vcat(b)):
        with pytest.raises(S.SpasmError):
            call()
    for x in (t, v, h, e, g):
        x.close()
        x.close()
