"""Dense triangular solves x T = b on the device (spasm_dense_forward_solve, spasm_dense_back_solve, the resident operator
spasm_amd_trsolve_* and S.TriangularSolver).  Every expected value comes from exact integer numpy or Python ints: products as
uint64 reduced per entry, the sequential loops of the reference restated in plain Python."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PRIMES = [3, 127, 42013, 65521, 2**31 - 1, 0xFFFFFFFB]


def bal(v, p):
    v = np.asarray(v, dtype=np.int64) % p
    return np.where(2 * v > p, v - p, v).astype(np.int32)


def csr_from_rows(S, n, m, rows, p):
    """rows[i]: list of (column, value) in storage order"""
    ptr = np.zeros(n + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    j = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    x = np.array([v for r in rows for _, v in r], dtype=np.int64)
    return S.CSR.from_arrays(n, m, ptr, j, bal(x, p) if len(x) else np.zeros(0, np.int32), prime=p)


def dense_of(T):
    k = int(T.p[T.n])
    D = np.zeros((T.n, T.m), dtype=np.int64)
    rows = np.repeat(np.arange(T.n), np.diff(np.asarray(T.p[: T.n + 1], dtype=np.int64)))
    np.add.at(D, (rows, T.j[:k].astype(np.int64)), T.x[:k].astype(np.int64))
    return D % T.prime


def xT(x, D, p):
    """x T mod p for a dense D (n x m, entries in [0, p)), exact: x (n,) or (n, k)"""
    x = np.asarray(x, dtype=np.int64) % p
    X = x[:, None] if x.ndim == 1 else x
    out = np.zeros((D.shape[1], X.shape[1]), dtype=np.int64)
    for i in np.flatnonzero(X.any(axis=1)):
        prod = (D[i].astype(np.uint64)[:, None] * X[i].astype(np.uint64)[None, :]) % np.uint64(p)
        out = (out + prod.astype(np.int64)) % p
    return out[:, 0] if x.ndim == 1 else out


def rand_tri(S, n, m, npart, p, rng, kind, density=0.3, triangular=False, diag=None):
    """A permuted triangular T.  Participating rows get ranks 0 .. npart-1 (a topological order); the row of rank r has entries on
    pivot columns of later ranks and on columns without a pivot, in shuffled order.  triangular=True stores it so that the
    reference's sequential loop applies: forward, rows in rank order; back, pivot columns decreasing with the rank.
    Returns (T, piv, rank_rows, rowcol)."""
    if triangular:
        part = np.arange(npart)
        pcols = np.sort(rng.choice(m, npart, replace=False))
        pcols = pcols[::-1] if kind == "back" else rng.permutation(pcols)
    else:
        part = rng.choice(n, npart, replace=False)
        pcols = rng.choice(m, npart, replace=False)
    rowcol = -np.ones(n, dtype=np.int64)
    rowcol[part] = pcols
    free = np.setdiff1d(np.arange(m), pcols)
    rows = [[] for _ in range(n)]
    for r, i in enumerate(part):
        later = pcols[r + 1 :]
        cols = list(later[rng.random(len(later)) < density]) + list(free[rng.random(len(free)) < density])
        d = 1 if kind == "forward" else int(rng.integers(1, p))
        if diag is not None:
            d = diag
        ent = [(int(c), int(rng.integers(1, p))) for c in cols] + [(int(pcols[r]), d)]
        rng.shuffle(ent)
        rows[i] = ent
    for i in np.setdiff1d(np.arange(n), part):  # non-participating rows: anything
        cols = np.flatnonzero(rng.random(m) < density)
        rows[i] = [(int(c), int(rng.integers(1, p))) for c in rng.permutation(cols)]
    T = csr_from_rows(S, n, m, rows, p)
    if kind == "forward":
        piv = rowcol.astype(np.int32)
    else:
        piv = -np.ones(m, dtype=np.int32)
        piv[pcols] = part
    return T, piv, part, rowcol


def solve(S, kind, T, b, x, piv):
    return (S.dense_forward_solve if kind == "forward" else S.dense_back_solve)(T, b, x, piv)


def seq_forward(U, b, q):
    """the reference's loop for x U = b (rows in storage order, unit pivots), Python ints"""
    p = U.prime
    b = [int(v) % p for v in b]
    x = [0] * U.n
    for i in range(U.n):
        j = int(q[i])
        if j < 0:
            continue
        if b[j] != 0:
            x[i] = b[j]
            for e in range(int(U.p[i]), int(U.p[i + 1])):
                c = int(U.j[e])
                b[c] = (b[c] - x[i] * int(U.x[e])) % p
    return bal(x, p), bal(b, p), all(v == 0 for v in b)


def seq_back(L, b, pv):
    """the reference's loop for x L = b (columns from the last, p[j] the row of column j's diagonal), Python ints"""
    p = L.prime
    b = [int(v) % p for v in b]
    x = [0] * L.n
    for j in range(L.m - 1, -1, -1):
        i = int(pv[j])
        if i < 0:
            continue
        lo, hi = int(L.p[i]), int(L.p[i + 1])
        d = sum(int(L.x[e]) for e in range(lo, hi) if int(L.j[e]) == j) % p
        x[i] = b[j] * pow(d, -1, p) % p
        for e in range(lo, hi):
            c = int(L.j[e])
            b[c] = (b[c] - x[i] * int(L.x[e])) % p
    return bal(x, p), bal(b, p), all(v == 0 for v in b)


def rand_int32(rng, shape):
    return rng.integers(-(2**31), 2**31, size=shape, dtype=np.int64).astype(np.int32)


@pytest.mark.parametrize("p", PRIMES)
@pytest.mark.parametrize("kind", ["forward", "back"])
def test_permuted_triangular_exact(S, p, kind):
    rng = np.random.default_rng(p % 100003 + (kind == "back"))
    n, m, npart = 70, 90, 55
    T, piv, part, rowcol = rand_tri(S, n, m, npart, p, rng, kind)
    D = dense_of(T)
    y = np.zeros(n, dtype=np.int64)
    y[part] = rng.integers(0, p, size=npart)
    b0 = bal(xT(y, D, p), p)
    b = b0.copy()
    x = rand_int32(rng, n)  # any int32 is accepted in x
    assert solve(S, kind, T, b, x, piv) is True
    assert np.array_equal(x, bal(y, p)) and not b.any()
    assert S._abi.last_error() == ""
    # unreduced b: same solution
    b = (b0.astype(np.int64) + p * rng.integers(-2, 3, size=m)).clip(-(2**31), 2**31 - 1).astype(np.int32)
    b = np.where(bal(b, p) == b0, b, b0).astype(np.int32)
    assert solve(S, kind, T, b, x, piv) and np.array_equal(x, bal(y, p))
    # perturbed off the pivot columns: same x, the perturbation is the residual
    free = np.setdiff1d(np.arange(m), rowcol[part])
    delta = np.zeros(m, dtype=np.int64)
    delta[rng.choice(free, 3, replace=False)] = rng.integers(1, p, size=3)
    b = bal(b0.astype(np.int64) + delta, p)
    assert solve(S, kind, T, b, x, piv) is False
    assert S._abi.last_error() == ""
    assert np.array_equal(x, bal(y, p)) and np.array_equal(b, bal(delta, p))
    # a random b: x exact on the pivot columns, b - x T exact
    bb = rand_int32(rng, m)
    b = bb.copy()
    ok = solve(S, kind, T, b, x, piv)
    res = bal(bb.astype(np.int64) - xT(x, D, p), p)
    assert np.array_equal(b, res) and not b[rowcol[part]].any() and ok == (not res.any())
    assert not x[np.setdiff1d(np.arange(n), part)].any()


@pytest.mark.parametrize("p", [3, 42013, 0xFFFFFFFB])
@pytest.mark.parametrize("kind", ["forward", "back"])
def test_triangular_order_matches_sequential_loop(S, p, kind):
    rng = np.random.default_rng(31 * p + (kind == "back"))
    n, m, npart = 60, 80, 50
    T, piv, part, rowcol = rand_tri(S, n, m, npart, p, rng, kind, density=0.25, triangular=True)
    D = dense_of(T)
    seq = seq_forward if kind == "forward" else seq_back
    y = np.zeros(n, dtype=np.int64)
    y[part] = rng.integers(0, p, size=npart)
    for b0 in (bal(xT(y, D, p), p), rand_int32(rng, m)):  # solvable, then (almost surely) unsolvable
        wx, wb, wok = seq(T, b0, piv)
        b, x = b0.copy(), np.zeros(n, dtype=np.int32)
        assert solve(S, kind, T, b, x, piv) == wok
        assert np.array_equal(x, wx) and np.array_equal(b, wb)


def test_factorizations_from_the_engine(S):
    rng = np.random.default_rng(5)
    for A in (S.synth_csr(0, 400, 300, density=0.01, prime=42013, seed=11), S.synth_csr(0, 3000, 2000, density=0.005, prime=42013, seed=12)):
        p = A.prime
        fact = S.echelonize(A)
        U = fact.U
        D = dense_of(U)
        with S.TriangularSolver.from_lu(fact) as ts:
            st = ts.stats()
            assert st["rows"] == fact.r == U.n
            y = rng.integers(0, p, size=U.n)
            b = bal(xT(y, D, p), p)
            X, ok = ts.solve(b)
            assert ok is True and np.array_equal(X, bal(y, p)) and not b.any()
            # the rows of A lie in the row space of U
            DA = dense_of(A)
            for i in rng.choice(A.n, 3, replace=False):
                b = bal(DA[i], p)
                X, ok = ts.solve(b)
                assert ok and not b.any()
                assert np.array_equal(bal(xT(X, D, p), p), bal(DA[i], p))
            # a vector outside it (when U does not have full column rank) is reported
            if fact.r < A.m:
                free = np.flatnonzero(np.asarray(fact.qinv) < 0)
                b = np.zeros(A.m, dtype=np.int32)
                b[free[0]] = 1
                X, ok = ts.solve(b)
                assert not ok and b[free[0]] == 1


def test_deep_chain_and_dense_triangle(S):
    p = 65521
    rng = np.random.default_rng(9)
    # bidiagonal chain of 200 000 rows: x_i + a_i x_{i-1} = b_i
    n = 200_000
    a = bal(rng.integers(1, p, size=n), p)
    ptr = np.arange(0, 2 * n + 1, 2, dtype=np.int64)
    j = np.empty(2 * n, dtype=np.int32)
    v = np.empty(2 * n, dtype=np.int32)
    j[0::2] = np.arange(n) + 1
    j[1::2] = np.arange(n)
    v[0::2] = a
    v[1::2] = 1
    U = S.CSR.from_arrays(n, n + 1, ptr, j, v, prime=p)
    q = np.arange(n, dtype=np.int32)
    b0 = bal(rng.integers(0, p, size=n + 1), p)
    wx, wb, wok = seq_forward(U, b0, q)
    b, x = b0.copy(), np.zeros(n, dtype=np.int32)
    with S.TriangularSolver(U, q) as ts:
        assert ts.stats()["levels"] == n
        X, ok = ts.solve(b)
    assert ok == wok and np.array_equal(X, wx) and np.array_equal(b, wb)
    # dense 2048 x 2048 triangle, back solve, rows shuffled
    n = 2048
    Lw = rng.integers(0, p, size=(n, n))
    Lw = np.tril(Lw, -1) + np.diag(rng.integers(1, p, size=n))
    perm = rng.permutation(n)
    Ls = Lw[perm]  # row r of the stored L is row perm[r] of Lw: diagonal on column perm[r]
    rows = [list(zip(np.flatnonzero(Ls[r]).tolist(), Ls[r][np.flatnonzero(Ls[r])].tolist())) for r in range(n)]
    L = csr_from_rows(S, n, n, rows, p)
    pv = np.empty(n, dtype=np.int32)
    pv[perm] = np.arange(n)
    b0 = bal(rng.integers(0, p, size=n), p)
    wx, wb, wok = seq_back(L, b0, pv)
    b, x = b0.copy(), np.zeros(n, dtype=np.int32)
    assert S.dense_back_solve(L, b, x, pv) == wok
    assert np.array_equal(x, wx) and np.array_equal(b, wb)


@pytest.mark.parametrize("p", [127, 65521, 0xFFFFFFFB])
def test_batches_equal_single_solves(S, p):
    rng = np.random.default_rng(p)
    n, m = 300, 340
    T, piv, part, rowcol = rand_tri(S, n, m, 280, p, rng, "forward", density=0.05)
    D = dense_of(T)
    with S.TriangularSolver(T, piv, "forward") as ts:
        for k in (1, 3, 8, 17, 64, 70):
            Y = np.zeros((n, k), dtype=np.int64)
            Y[part] = rng.integers(0, p, size=(len(part), k))
            B0 = bal(xT(Y, D, p), p)
            B0[:, ::2] = rand_int32(rng, (m, (k + 1) // 2))  # every other vector unsolvable
            big = np.full((m, k + 5), 7, dtype=np.int32)  # ld > k
            big[:, :k] = B0
            Xbig = np.full((n, k + 3), 9, dtype=np.int32)
            B = big[:, :k]
            X, ok = ts.solve(B, Xbig[:, :k])
            assert (big[:, k:] == 7).all() and (Xbig[:, k:] == 9).all()
            for v in range(k):
                bv, xv = B0[:, v].copy(), np.zeros(n, dtype=np.int32)
                okv = S.dense_forward_solve(T, bv, xv, piv)
                assert okv == ok[v] and np.array_equal(xv, X[:, v]) and np.array_equal(bv, B[:, v]), (k, v)
            assert ok[1::2].all() if k > 1 else True


def test_torch_on_a_side_stream(S):
    import torch

    p = 42013
    rng = np.random.default_rng(3)
    n, m, k = 500, 520, 8
    T, piv, part, rowcol = rand_tri(S, n, m, 450, p, rng, "back", density=0.03)
    D = dense_of(T)
    Y = np.zeros((n, k), dtype=np.int64)
    Y[part] = rng.integers(0, p, size=(len(part), k))
    B0 = bal(xT(Y, D, p), p)
    B0[:, 0] = rand_int32(rng, m)
    with S.TriangularSolver(T, piv, kind="back") as ts:
        Bh = B0.copy()
        Xh, okh = ts.solve(Bh)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            B = torch.from_numpy(B0.copy()).cuda()
            X, ok = ts.solve(B)
            Xc, okc, Bc = X.cpu().numpy(), ok.cpu().numpy(), B.cpu().numpy()
        s.synchronize()
    assert np.array_equal(Xc, Xh) and np.array_equal(okc, okh) and np.array_equal(Bc, Bh)
    assert okh[1:].all() and np.array_equal(Xh[:, 1:], bal(Y[:, 1:], p))


def test_errors_leave_b_and_x_unchanged(S):
    p = 42013
    cases = []
    # cycle: row 0 has an entry on row 1's pivot column and row 1 on row 0's
    cases.append(("forward", 2, 2, [[(0, 1), (1, 5)], [(1, 1), (0, 3)]], [0, 1], "cycle"))
    cases.append(("forward", 2, 3, [[(0, 1)], [(0, 1)]], [0, 0], "pivot of rows"))       # duplicate pivot
    cases.append(("forward", 2, 3, [[(0, 1)], [(1, 2)]], [0, 1], "not 1"))               # non-unit pivot
    cases.append(("forward", 2, 3, [[(0, 1)], [(2, 1)]], [0, 3], "out of range"))        # pivot out of range
    cases.append(("back", 2, 3, [[(0, 4)], [(1, 3)]], [0, 0, -1], "holds the pivots"))   # row claimed twice
    cases.append(("back", 2, 3, [[(0, 4)], [(2, 3)]], [0, 1, -1], "zero"))               # zero diagonal (no entry on column 1)
    cases.append(("back", 2, 2, [[(0, 4), (1, 1)], [(1, 3), (0, 2)]], [0, 1], "cycle"))
    for kind, n, m, rows, piv, what in cases:
        T = csr_from_rows(S, n, m, rows, p)
        piv = np.array(piv, dtype=np.int32)
        with pytest.raises(S.SpasmError, match=what):
            S.TriangularSolver(T, piv, kind)
        b = np.array([5, -7, 2**31 - 1][:m], dtype=np.int32)
        x = np.array([-(2**31), 3][:n], dtype=np.int32)
        b0, x0 = b.copy(), x.copy()
        with pytest.raises(S.SpasmError, match=what):
            solve(S, kind, T, b, x, piv)
        assert np.array_equal(b, b0) and np.array_equal(x, x0), (kind, what)
        lib = S._abi.lib()
        sym = lib.spasm_dense_forward_solve if kind == "forward" else lib.spasm_dense_back_solve
        assert sym(T.data, b.ctypes.data, x.ctypes.data, piv.ctypes.data) is False
        assert what in S._abi.last_error()
        assert np.array_equal(b, b0) and np.array_equal(x, x0)


def test_empty_cases(S):
    p = 127
    for n, m, rows in ((0, 4, []), (3, 0, [[], [], []]), (3, 4, [[], [], []]), (0, 0, [])):
        T = csr_from_rows(S, n, m, rows, p)
        b = np.array([1, 0, -3, 200][:m], dtype=np.int32)
        x = np.full(n, 5, dtype=np.int32)
        q = np.full(n, -1, dtype=np.int32)
        ok = S.dense_forward_solve(T, b, x, q)
        assert ok == (not bal(b, p).any() if m else True)
        assert not x.any() and np.array_equal(b, bal(np.array([1, 0, -3, 200][:m]), p))
        pv = np.full(m, -1, dtype=np.int32)
        assert S.dense_back_solve(T, b, x, pv) == ok
    # participating rows without other entries: x = b on the pivot columns
    T = csr_from_rows(S, 2, 3, [[(2, 1)], [(0, 1)]], p)
    b = np.array([4, 0, -6], dtype=np.int32)
    x = np.zeros(2, dtype=np.int32)
    assert S.dense_forward_solve(T, b, x, np.array([2, 0], dtype=np.int32))
    assert x.tolist() == [-6, 4] and not b.any()
    with S.TriangularSolver(T, np.array([2, 0], dtype=np.int32)) as ts:
        X, ok = ts.solve(np.zeros((3, 0), dtype=np.int32))
        assert X.shape == (2, 0) and ok.shape == (0,)
