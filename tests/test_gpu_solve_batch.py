"""X * A = B for many small systems (S.solve_batch) and block by block (S.DeviceBlocks.solve, S.blocks.solve) against exact integer
arithmetic on the host, written here: a Gauss-Jordan elimination of [A^T | B^T] mod p in int64 (p < 2^31: products stay below
2^62) or in numpy object arrays of Python ints (p >= 2^31).  It gives the canonical row basis (row j of A belongs to it iff it is no
combination of rows 0 .. j-1: the pivot columns of the reduced form of A^T, which do not depend on the order of elimination), the
solvable right-hand sides, and the one solution that lives on that basis.  Every X is also multiplied back: X * A == B mod p."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PRIMES = [3, 7, 127, 42013, 65521, 2147483647, 4294967291]


# ---------------------------------------------------------------------------------------------------------------------------------
# the host side
# ---------------------------------------------------------------------------------------------------------------------------------
def host_solve(A, B, p):
    """A (n x m), B (K x m): integer arrays with entries in [0, p).  Returns (X, ok, basis): X (K x n, entries in [0, p), zero rows
    where ok is False), ok (K bools), basis (the rows of A of the canonical basis, ascending)."""
    big = p >= 2 ** 31
    dt = object if big else np.int64
    n, m = A.shape
    K = B.shape[0]
    T = np.concatenate([A.T.astype(dt), B.T.astype(dt)], axis=1) if m else np.zeros((0, n + K), dtype=dt)
    free = np.ones(m, dtype=bool)
    piv = []
    for c in range(n):
        cand = np.nonzero(free & (T[:, c] != 0))[0] if m else []
        if len(cand) == 0:
            continue
        r = int(cand[-1])  # (any candidate will do: the reduced form is unique)
        T[r] = (T[r] * pow(int(T[r, c]), -1, p)) % p
        f = T[:, c].copy()
        f[r] = 0
        T = (T - np.outer(f, T[r])) % p
        free[r] = False
        piv.append((r, c))
    ok = np.array([not np.any(T[free, n + t] != 0) for t in range(K)], dtype=bool)
    X = np.zeros((K, n), dtype=dt)
    for t in range(K):
        if ok[t]:
            for r, c in piv:
                X[t, c] = T[r, n + t]
    return X, ok, [c for _, c in piv]


def bal(v, p):
    v = int(v) % p
    return v - p if 2 * v > p else v


def make_csr(S, D, p, rng, messy=True):
    """the CSR of the dense D (entries in [0, p)).  messy: entries of a row in random order, values moved by multiples of p where
    int32 allows, balanced or not, and explicit zeros (0 or a multiple of p) on some empty places.  Not messy: columns ascending
    and balanced values, which every p <= 0xFFFFFFFB keeps inside int32 and which echelonize and gesv expect."""
    n, m = D.shape
    pp, jj, xx = [0], [], []
    for i in range(n):
        ent = [(c, int(D[i, c]) if messy else bal(D[i, c], p)) for c in range(m) if D[i, c] != 0]
        if messy:
            zeros = [c for c in range(m) if D[i, c] == 0]
            for c in zeros[: int(rng.integers(0, 3))] if rng.random() < 0.4 else []:
                ent.append((c, 0))
            out = []
            for c, v in ent:
                choices = [v, v - p]
                for k in (-3, 2, 5):
                    if -2 ** 31 <= v + k * p < 2 ** 31:
                        choices.append(v + k * p)
                choices = [w for w in choices if -2 ** 31 <= w < 2 ** 31]
                out.append((c, int(choices[int(rng.integers(0, len(choices)))])))
            ent = [out[q] for q in rng.permutation(len(out))]
        jj += [c for c, _ in ent]
        xx += [v for _, v in ent]
        pp.append(len(jj))
    return S.CSR.from_arrays(n, m, np.array(pp, dtype=np.int64), np.array(jj, dtype=np.int32), np.array(xx, dtype=np.int64).astype(np.int32), prime=p)


def raw(X):
    """the bytes of a CSR that the contract speaks of"""
    nz = int(X.p[X.n])
    return (X.shape, X.prime, X.nzmax, X.p.tolist(), X.j[:nz].tolist(), X.x[:nz].tolist())


def check_canonical(X, p):
    nz = int(X.p[X.n])
    assert X.nzmax == nz, (X.nzmax, nz)
    x = X.x[:nz].astype(np.int64)
    assert np.all(x != 0) and np.all(x >= p // 2 - p + 1) and np.all(x <= p // 2)
    for k in range(X.n):
        row = X.j[int(X.p[k]):int(X.p[k + 1])]
        assert np.all(np.diff(row) > 0) and (len(row) == 0 or (row[0] >= 0 and row[-1] < X.m))


def check_system(X, ok, A, B, p, canonical=True):
    """the result of one system against host_solve(A, B): ok exactly; on the LDS path X entry for entry, on the general path
    X * A == B on the solvable rows and empty rows elsewhere"""
    Xw, okw, _ = host_solve(A, B, p)
    assert ok.tolist() == okw.tolist()
    assert X.shape == (B.shape[0], A.shape[0]) and X.prime == p
    check_canonical(X, p)
    rows = X.rows()
    big = p >= 2 ** 31
    Ao = A.astype(object) if big else A.astype(np.int64)
    for k in range(B.shape[0]):
        if not okw[k]:
            assert rows[k] == []
            continue
        if canonical:
            assert rows[k] == [(c, bal(Xw[k, c], p)) for c in range(A.shape[0]) if Xw[k, c] != 0], k
        acc = np.zeros(A.shape[1], dtype=object if big else np.int64)
        for c, v in rows[k]:
            acc = (acc + (v % p) * Ao[c]) % p
        assert np.array_equal(acc, B[k] % p), k
    return int((~okw).sum())


def random_system(rng, n, m, K, p, density, planted=True):
    """A with planted dependent rows (a combination of two others, before and after them), zero rows and zero columns; half of the
    right-hand sides are y * A, half random"""
    A = ((rng.random((n, m)) < density) * rng.integers(1, p, size=(n, m))).astype(object)
    if planted and n >= 4:
        a, b = 1, n - 2
        A[0] = (int(rng.integers(1, p)) * A[a] + int(rng.integers(1, p)) * A[b]) % p      # before the two
        A[n - 1] = (int(rng.integers(1, p)) * A[a] + int(rng.integers(1, p)) * A[b]) % p  # after them
        if n >= 6:
            A[n // 2] = 0
    if planted and m >= 3:
        A[:, int(rng.integers(0, m))] = 0
    B = np.zeros((K, m), dtype=object)
    kind = []
    for k in range(K):
        if k % 2 == 0:
            y = rng.integers(0, p, size=n).astype(object) * (rng.random(n) < 0.6)
            B[k] = (y @ A) % p if n else 0
            kind.append("image")
        elif rng.random() < 0.15:
            kind.append("empty")
        else:
            B[k] = rng.integers(0, p, size=m).astype(object) * (rng.random(m) < max(density, 0.3))
            kind.append("random")
    dt = object if p >= 2 ** 31 else np.int64
    return A.astype(dt), B.astype(dt), kind


def solve_one(S, A, B, p, seed=0, messy=True):
    rng = np.random.default_rng(seed)
    X, ok = S.solve_batch([make_csr(S, A, p, rng, messy)], [make_csr(S, B, p, rng, messy)])
    return X[0], ok[0]


def dense(rows, n, m, dt=np.int64):
    D = np.zeros((n, m), dtype=dt)
    for i, r in enumerate(rows):
        for c, v in r:
            D[i, c] = v
    return D


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the sweep
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    rng = np.random.default_rng(20260117)
    cases = []
    for t in range(150):
        p = PRIMES[t % len(PRIMES)]
        n, m, K = int(rng.integers(1, 57)), int(rng.integers(1, 57)), int(rng.integers(1, 9))
        density = [0.05, 0.1, 0.25, 0.5, 1.0][t % 5]
        A, B, kind = random_system(rng, n, m, K, p, density)
        Xw, okw, basis = host_solve(A, B, p)
        cases.append((A, B, p, kind, okw))
    rand = [o for c in cases for k, o in zip(c[3], c[4]) if k == "random"]
    every = [o for c in cases for o in c[4]]
    # an all-ok or an all-fail implementation cannot pass
    assert sum(not o for o in rand) * 4 >= len(rand), (sum(not o for o in rand), len(rand))
    assert sum(bool(o) for o in every) * 4 >= len(every)
    return cases


def test_sweep_against_the_host_elimination(S, sweep):
    rng = np.random.default_rng(5)
    As = [make_csr(S, c[0], c[2], rng) for c in sweep]
    Bs = [make_csr(S, c[1], c[2], rng) for c in sweep]
    X, ok = S.solve_batch(As, Bs)
    st = S.solve_stats()
    unsolved = 0
    for (A, B, p, _, _), x, o in zip(sweep, X, ok):
        unsolved += check_system(x, o, A, B, p)
    assert st["systems"] == len(sweep) and st["lds_path"] == len(sweep) and st["general_path"] == 0
    assert st["unsolved"] == unsolved and st["jobs"] == len(sweep) and st["entries"] == sum(S.nnz(x) for x in X)
    assert 1 <= st["launches"] <= 6  # at most four eliminations, a scan and a pack: one chunk
    # two runs are byte-identical
    X2, ok2 = S.solve_batch(As, Bs)
    assert [raw(x) for x in X2] == [raw(x) for x in X] and [o.tolist() for o in ok2] == [o.tolist() for o in ok]


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. corners
# ---------------------------------------------------------------------------------------------------------------------------------
def test_corner_one_by_one(S):
    p = 127
    X, ok = solve_one(S, np.array([[5]]), np.array([[0], [10], [3]]), p)
    assert ok.tolist() == [True, True, True] and X.rows() == [[], [(0, 2)], [(0, bal(3 * pow(5, -1, p), p))]]
    X, ok = solve_one(S, np.array([[0]]), np.array([[0], [4]]), p)
    assert ok.tolist() == [True, False] and X.rows() == [[], []]


def test_corner_single_row_and_single_column(S):
    p = 42013
    rng = np.random.default_rng(1)
    A = rng.integers(0, p, size=(1, 9))
    B = np.stack([(7 * A[0]) % p, rng.integers(0, p, size=9), np.zeros(9, dtype=np.int64)])
    X, ok = solve_one(S, A, B, p)
    assert check_system(X, ok, A, B, p) == 1 and X.rows()[0] == [(0, 7)]
    A = np.array([[0], [3], [6], [0], [1]])  # n x 1: the basis is the first non-zero row
    B = np.array([[5], [0]])
    X, ok = solve_one(S, A, B, p)
    assert check_system(X, ok, A, B, p) == 0 and X.rows() == [[(1, bal(5 * pow(3, -1, p), p))], []]


def test_corner_no_rows_no_columns_no_right_hand_sides(S):
    p = 7
    X, ok = S.solve_batch([S.CSR.from_rows([], 2, prime=p)], [S.CSR.from_arrays(3, 2, [0, 0, 1, 2], [1, 0], [7, 3], prime=p)])
    assert ok[0].tolist() == [True, True, False] and X[0].shape == (3, 0) and S.nnz(X[0]) == 0
    X, ok = S.solve_batch([S.CSR.from_rows([[], [], []], 0, prime=p)], [S.CSR.from_rows([[], []], 0, prime=p)])
    assert ok[0].tolist() == [True, True] and X[0].shape == (2, 3) and S.nnz(X[0]) == 0
    X, ok = S.solve_batch([S.CSR.from_rows([[(0, 1)]], 2, prime=p)], [S.CSR.from_rows([], 2, prime=p)])
    assert ok[0].tolist() == [] and X[0].shape == (0, 1)
    assert S.solve_stats()["launches"] == 0 and S.solve_stats()["lds_path"] == 1


def test_corner_all_rows_equal_use_row_zero_only(S):
    p = 65521
    A = np.tile(np.array([[3, 0, 5, 7]]), (6, 1))
    B = np.array([[6, 0, 10, 14], [3, 1, 5, 7]])
    X, ok = solve_one(S, A, B, p)
    assert ok.tolist() == [True, False] and X.rows() == [[(0, 2)], []]
    assert host_solve(A, B, p)[2] == [0]


def test_corner_reversed_identity(S):
    p = 4294967291
    n = 9
    A = np.zeros((n, n), dtype=object)
    for i in range(n):
        A[i, n - 1 - i] = 1
    B = np.array([[(3 * c + 1) % p for c in range(n)], [p - 1 - c for c in range(n)]], dtype=object)
    X, ok = solve_one(S, A, B, p)
    assert check_system(X, ok, A, B, p) == 0
    assert X.rows()[0] == [(i, bal(3 * (n - 1 - i) + 1, p)) for i in range(n)]


def test_corner_singular_square_matrices_use_the_canonical_basis(S):
    """Singular square matrices in which a right-hand side has several solutions; only the one on the canonical basis may come
    back.  In the first, rows 0 and 1 are parallel and b needs the LAST row: the basis is {0, 2}, and (1, 4, 0) = 4 * row 0 + row 2
    (not 2 * row 1 + row 2).  In the second the parallel rows share column 0 with the last row, which the election of a column-wise
    elimination of A would never take for that column: (5, 1, 0) = 2 * row 0 + row 2 (not row 1 + row 2)."""
    p = 127
    A = np.array([[0, 1, 0], [0, 2, 0], [1, 0, 0]])
    B = np.array([[1, 0, 0], [1, 4, 0], [0, 0, 1]])
    X, ok = solve_one(S, A, B, p)
    assert host_solve(A, B, p)[2] == [0, 2]
    assert ok.tolist() == [True, True, False]
    assert X.rows() == [[(2, 1)], [(0, 4), (2, 1)], []]
    A = np.array([[1, 0, 0], [2, 0, 0], [3, 1, 0]])
    B = np.array([[5, 1, 0]])
    X, ok = solve_one(S, A, B, p)
    assert host_solve(A, B, p)[2] == [0, 2] and ok.tolist() == [True] and X.rows() == [[(0, 2), (2, 1)]]


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. shapes that stress the kernel
# ---------------------------------------------------------------------------------------------------------------------------------
SHAPES = [
    (3, 600, 5, 65521),      # more image rows than threads: the election loops over bases
    (60, 20, 3, 127), (60, 20, 4, 127), (60, 20, 5, 127),          # n + w = 63, 64, 65
    (120, 20, 7, 42013), (120, 20, 8, 42013), (120, 20, 9, 42013),  # n + w = 127, 128, 129
    (37, 30, 2, 7), (37, 31, 2, 7), (38, 30, 2, 7), (38, 31, 2, 7),  # m even / odd, n + w odd / even (stride padding)
    (32, 31, 1, 3), (31, 32, 1, 3), (40, 25, 1, 3),                # image words 1023, 1024 (no room for the padding), 1025
    (64, 63, 1, 65521), (63, 64, 1, 65521), (240, 17, 1, 65521),   # 4095, 4096, 4097
    (137, 89, 1, 2147483647), (127, 96, 1, 2147483647), (1117, 11, 1, 2147483647),  # 12282, 12288, 12298
    (181, 180, 2, 65521),    # m * (n + 1) = 32760: the last LDS shape
]


@pytest.mark.parametrize("n,m,K,p", SHAPES)
def test_shapes(S, n, m, K, p):
    rng = np.random.default_rng(n * 1000 + m)
    A, B, _ = random_system(rng, n, m, K, p, 0.5 if n * m < 20000 else 0.2)
    X, ok = solve_one(S, A, B, p, messy=n * m < 5000)
    check_system(X, ok, A, B, p)
    st = S.solve_stats()
    assert st["general_path"] == 0 and st["lds_path"] == 1 and st["jobs"] == 1


def test_first_general_path_shape(S):
    p, n, m = 65521, 181, 181  # m * (n + 1) = 32942
    rng = np.random.default_rng(9)
    A, B, _ = random_system(rng, n, m, 4, p, 0.1)
    X, ok = solve_one(S, A, B, p, messy=False)
    check_system(X, ok, A, B, p, canonical=False)
    st = S.solve_stats()
    assert st["general_path"] == 1 and st["lds_path"] == 0 and st["jobs"] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. slabs
# ---------------------------------------------------------------------------------------------------------------------------------
def test_slabs_do_not_show_in_the_result(S):
    p, n, K = 65521, 100, 700
    rng = np.random.default_rng(4)
    A = rng.integers(0, p, size=(n, n))
    A[70:] = (rng.integers(0, p, size=(30, 70)) @ A[:70]) % p  # rank 70
    Y = rng.integers(0, p, size=(K, n))
    B = (Y @ A) % p
    B[1::2] = rng.integers(0, p, size=(K // 2, n))
    Ac, Bc = make_csr(S, A, p, rng, False), make_csr(S, B, p, rng, False)
    X, ok = S.solve_batch([Ac], [Bc])
    st = S.solve_stats()
    assert st["systems"] == 1 and st["jobs"] > 1 and st["unsolved"] == K // 2
    check_system(X[0], ok[0], A, B, p)
    halves = [S.solve_batch([Ac], [make_csr(S, B[lo:lo + 350], p, rng, False)]) for lo in (0, 350)]
    nz0 = S.nnz(halves[0][0][0])
    both = (X[0].shape, p, S.nnz(X[0]),
            halves[0][0][0].p.tolist() + [nz0 + v for v in halves[1][0][0].p.tolist()[1:]],
            halves[0][0][0].j[:nz0].tolist() + halves[1][0][0].j[:S.nnz(halves[1][0][0])].tolist(),
            halves[0][0][0].x[:nz0].tolist() + halves[1][0][0].x[:S.nnz(halves[1][0][0])].tolist())
    assert raw(X[0]) == both
    assert ok[0].tolist() == halves[0][1][0].tolist() + halves[1][1][0].tolist()
    X2, ok2 = S.solve_batch([Ac], [Bc])
    assert raw(X2[0]) == raw(X[0]) and ok2[0].tolist() == ok[0].tolist()


def test_small_scratch_budget_solves_in_chunks(S, monkeypatch):
    """60 systems of 20 x 20 with 8 right-hand sides, every third one singular: a job needs about 2.9 KB of the chunk's buffers, so a
    budget of 0.05 MB cuts the call into three chunks or more, and nothing of that may show in the result."""
    p, n, K = 65521, 20, 8
    rng = np.random.default_rng(60)
    sys = [random_system(rng, n, n, K, p, 0.5, planted=t % 3 == 0) for t in range(60)]
    unsolved = sum(int((~host_solve(A, B, p)[1]).sum()) for A, B, _ in sys)
    assert 0 < unsolved < 60 * K // 2
    As = [make_csr(S, A, p, rng) for A, _, _ in sys]
    Bs = [make_csr(S, B, p, rng) for _, B, _ in sys]
    X, ok = S.solve_batch(As, Bs)
    whole = S.solve_stats()
    assert whole["lds_path"] == 60 and whole["unsolved"] == unsolved
    monkeypatch.setenv("SPASM_AMD_BATCH_SCRATCH_MB", "0.05")
    Xc, okc = S.solve_batch(As, Bs)
    cut = S.solve_stats()
    print("solve_stats", whole, cut)
    assert [raw(x) for x in Xc] == [raw(x) for x in X] and [o.tolist() for o in okc] == [o.tolist() for o in ok]
    assert cut["jobs"] == whole["jobs"] and cut["entries"] == whole["entries"]
    assert cut["launches"] > whole["launches"]  # every chunk costs an elimination and a scan at the least
    monkeypatch.delenv("SPASM_AMD_BATCH_SCRATCH_MB")
    S.solve_batch(As[:3], Bs[:3])
    assert S.solve_stats()["launches"] == whole["launches"]


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. a mixed batch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_mixed_batch_keeps_the_input_order(S):
    rng = np.random.default_rng(6)
    spec = [(5, 7, 3, 127), (200, 170, 2, 65521), (30, 30, 8, 4294967291), (0, 4, 2, 7), (181, 181, 1, 42013), (12, 50, 4, 3), (50, 12, 4, 2147483647)]
    sys = [random_system(rng, n, m, K, p, 0.3)[:2] + (p,) for n, m, K, p in spec]
    X, ok = S.solve_batch([make_csr(S, A, p, rng, A.size < 5000) for A, _, p in sys], [make_csr(S, B, p, rng, A.size < 5000) for A, B, p in sys])
    st = S.solve_stats()
    unsolved = 0
    for (A, B, p), x, o, (n, m, K, _) in zip(sys, X, ok, spec):
        unsolved += check_system(x, o, A, B, p, canonical=m * (n + 1) <= 32768)
    assert (st["systems"], st["lds_path"], st["general_path"], st["jobs"], st["unsolved"]) == (7, 5, 2, 4, unsolved)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. blocks
# ---------------------------------------------------------------------------------------------------------------------------------
def block_matrix(S, rng, shapes, p, empty_rows=3, empty_cols=3):
    """the shuffled direct sum of random connected blocks of the given shapes, plus empty rows and columns; returns the dense matrix"""
    n = sum(a for a, _ in shapes) + empty_rows
    m = sum(b for _, b in shapes) + empty_cols
    D = np.zeros((n, m), dtype=np.int64)
    r0 = c0 = 0
    for a, b in shapes:
        Bk = (rng.random((a, b)) < 0.5) * rng.integers(1, p, size=(a, b))
        for i in range(a):  # a path through the block keeps it connected
            Bk[i, i % b] = Bk[i, i % b] or 1
            if i + 1 < a:
                Bk[i + 1, i % b] = Bk[i + 1, i % b] or 2
        for c in range(b):
            Bk[c % a, c] = Bk[c % a, c] or 3
        if a >= 3:
            Bk[a - 1] = (Bk[0] + 2 * Bk[1]) % p
            for c in range(b):
                if not Bk[:, c].any():
                    Bk[0, c] = 1
        D[r0:r0 + a, c0:c0 + b] = Bk
        r0 += a
        c0 += b
    return D[rng.permutation(n)][:, rng.permutation(m)]


def block_rhs(rng, D, p, K):
    """rows built as y * A (with y on one row of A, or on many), random sparse rows, entries on empty columns, empty rows"""
    n, m = D.shape
    empty_cols = np.nonzero(~D.any(axis=0))[0]
    B = np.zeros((K, m), dtype=np.int64)
    for k in range(K):
        kind = k % 6
        if kind in (0, 1, 2):
            y = np.zeros(n, dtype=np.int64)
            pick = rng.choice(n, size=1 if kind == 0 else min(n, 25), replace=False)
            y[pick] = rng.integers(1, p, size=len(pick))
            B[k] = (y @ D) % p
            if kind == 2 and len(empty_cols):
                B[k, empty_cols[0]] = 1 + int(rng.integers(0, p - 1))   # unsolvable through the empty column alone
        elif kind == 3:
            cols = rng.choice(m, size=min(m, 6), replace=False)
            B[k, cols] = rng.integers(0, p, size=len(cols))
        elif kind == 4:
            c = int(rng.integers(0, m))
            B[k, c] = int(rng.integers(1, p))
    return B


def rhs_csr(S, B, D, p, rng):
    """B as a CSR with shuffled rows, plus a stored zero on an empty column of A here and there"""
    X = make_csr(S, B, p, rng, messy=False)
    empty_cols = np.nonzero(~D.any(axis=0))[0]
    rows = []
    for k in range(B.shape[0]):
        r = [(c, int(B[k, c])) for c in rng.permutation(B.shape[1]) if B[k, c]]
        if k % 3 == 0 and len(empty_cols) and B[k, empty_cols[-1]] == 0:
            r.insert(len(r) // 2, (int(empty_cols[-1]), 0))
        rows.append(r)
    pp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return S.CSR.from_arrays(B.shape[0], B.shape[1], pp, [c for r in rows for c, _ in r], [v for r in rows for _, v in r], prime=X.prime)


def times_A(X, D, p):
    """X * A mod p, dense, from the rows of X"""
    out = np.zeros((X.n, D.shape[1]), dtype=np.int64)
    for k, r in enumerate(X.rows()):
        for c, v in r:
            out[k] = (out[k] + (v % p) * D[c]) % p
    return out


def test_blocks_three_routes_agree_byte_for_byte(S):
    """As many components of 1 x 1 .. 12 x 14 as the LDS limit admits for the matrix as a whole (m * (n + 1) <= 32768 is what lets
    solve_batch take A as one system): the device split, the unsplit matrix and the host split must return the same bytes."""
    p = 42013
    rng = np.random.default_rng(31)
    shapes, n, m = [], 3, 3
    while True:
        a, b = (int(rng.integers(1, 13)), int(rng.integers(1, 15))) if len(shapes) % 9 == 0 else (int(rng.integers(1, 4)), int(rng.integers(1, 4)))
        if (m + b) * (n + a + 1) > 32768:
            break
        shapes.append((a, b))
        n, m = n + a, m + b
    D = block_matrix(S, rng, shapes, p)
    assert D.shape == (n, m) and m * (n + 1) <= 32768 and len(shapes) > 60
    A = make_csr(S, D, p, rng, messy=False)
    B = block_rhs(rng, D, p, 48)
    Bc = rhs_csr(S, B, D, p, rng)
    with S.DeviceBlocks(A) as Dev:
        assert len(Dev) == len(shapes) + 6
        Xd, okd = Dev.solve(Bc)
        st = S.solve_stats()
        Xd2, okd2 = S.blocks.solve(Dev, Bc)
    Xa, oka = S.solve_batch([A], [Bc])
    Xh, okh = S.blocks.solve(S.Block.from_csr(A), Bc)
    assert raw(Xd) == raw(Xa[0]) == raw(Xh) == raw(Xd2)
    assert okd.tolist() == oka[0].tolist() == okh.tolist() == okd2.tolist()
    unsolved = check_system(Xd, okd, D, B, p)
    assert 0 < unsolved < 48 and st["unsolved"] == unsolved and st["general_path"] == 0 and st["entries"] == S.nnz(Xd)
    assert not okd[2]  # the entry on an empty column


def test_blocks_many_components(S):
    p = 65521
    rng = np.random.default_rng(32)
    shapes = [(int(rng.integers(1, 13)), int(rng.integers(1, 15))) for _ in range(3000)]
    n, m = sum(a for a, _ in shapes) + 3, sum(b for _, b in shapes) + 3
    # built sparse: the dense matrix would hold half a billion cells
    rperm, cperm = rng.permutation(n), rng.permutation(m)
    rows = [[] for _ in range(n)]
    r0 = c0 = 0
    for a, b in shapes:
        Bk = block_matrix(S, rng, [(a, b)], p, 0, 0)
        for i in range(a):
            rows[rperm[r0 + i]] = [(int(cperm[c0 + c]), int(Bk[i, c])) for c in range(b) if Bk[i, c]]
        r0, c0 = r0 + a, c0 + b
    A = S.CSR.from_rows(rows, m, prime=p)
    import scipy.sparse as sp

    Asp = sp.csr_matrix((A.x[:S.nnz(A)].astype(np.int64) % p, A.j[:S.nnz(A)], A.p), shape=(n, m))
    K = 40
    brows = []
    for k in range(K):
        y = sp.csr_matrix((rng.integers(1, p, size=30), (np.zeros(30, dtype=np.int64), rng.choice(n, size=30, replace=False))), shape=(1, n))
        b = np.asarray((y @ Asp).todense()).ravel() % p
        if k % 4 == 3:
            b[rng.choice(m, size=3)] += 1
        brows.append([(int(c), int(b[c] % p)) for c in np.nonzero(b % p)[0]])
    Bc = S.CSR.from_rows(brows, m, prime=p)
    with S.DeviceBlocks(A) as Dev:
        Xd, okd = Dev.solve(Bc)
        st = S.solve_stats()
    Xh, okh = S.blocks.solve(S.Block.from_csr(A), Bc)
    assert raw(Xd) == raw(Xh) and okd.tolist() == okh.tolist()
    assert okd[:3].all() and 0 < (~okd).sum() <= K // 4 and st["general_path"] == 0 and st["lds_path"] == st["systems"] > 100
    check_canonical(Xd, p)
    Xsp = sp.csr_matrix((Xd.x[:S.nnz(Xd)].astype(np.int64) % p, Xd.j[:S.nnz(Xd)], Xd.p), shape=(K, n))
    got = np.asarray((Xsp @ Asp).todense()) % p
    want = np.asarray(sp.csr_matrix((Bc.x[:S.nnz(Bc)].astype(np.int64) % p, Bc.j[:S.nnz(Bc)], Bc.p), shape=(K, m)).todense())
    for k in range(K):
        if okd[k]:
            assert np.array_equal(got[k], want[k]), k
        else:
            assert Xd.rows()[k] == []


def test_blocks_from_a_resident_matrix(S):
    p = 127
    rng = np.random.default_rng(33)
    D = block_matrix(S, rng, [(4, 5), (1, 1), (6, 3), (2, 2), (3, 7)], p)
    A = make_csr(S, D, p, rng, messy=False)
    B = block_rhs(rng, D, p, 18)
    Bc = rhs_csr(S, B, D, p, rng)
    with S.DeviceCSR(A) as R, S.DeviceBlocks(R) as Dev:
        X, ok = Dev.solve(Bc)
    check_system(X, ok, D, B, p)
    Xa, oka = S.solve_batch([A], [Bc])
    assert raw(X) == raw(Xa[0]) and ok.tolist() == oka[0].tolist()


def test_blocks_one_component_over_the_limit(S):
    p = 65521
    rng = np.random.default_rng(34)
    D = block_matrix(S, rng, [(3, 4), (190, 190), (2, 2), (5, 3)], p)
    A = make_csr(S, D, p, rng, messy=False)
    B = block_rhs(rng, D, p, 12)
    with S.DeviceBlocks(A) as Dev:
        X, ok = Dev.solve(rhs_csr(S, B, D, p, rng))
        st = S.solve_stats()
    assert st["general_path"] == 1 and st["lds_path"] >= 3
    check_system(X, ok, D, B, p, canonical=False)


def test_blocks_errors_against_a_live_handle(S):
    import ctypes as C

    p = 127
    A = S.CSR.from_rows([[(0, 1), (1, 2)], [(2, 3)]], 4, prime=p)
    with S.DeviceBlocks(A) as Dev:
        fn = S._abi.lib().spasm_amd_blocks_solve
        out = C.POINTER(S._abi.CsrStruct)()
        C.cast(C.pointer(out), C.POINTER(C.c_uint64))[0] = 0x5A5A5A5A
        okb = np.full(2, 0xA5, dtype=np.uint8)
        okp = okb.ctypes.data_as(C.POINTER(C.c_ubyte))

        def untouched():
            return C.cast(C.pointer(out), C.POINTER(C.c_uint64))[0] == 0x5A5A5A5A and (okb == 0xA5).all()

        for Rhs, text in ((S.CSR.from_rows([[(0, 1)], []], 4, prime=7), "prime"), (S.CSR.from_rows([[(0, 1)], []], 5, prime=p), "Rhs->m")):
            assert fn(Dev._need(), Rhs.data, C.byref(out), okp) == -1
            assert S._abi.last_error().startswith("spasm_amd_blocks_solve") and text in S._abi.last_error()
            assert untouched()
        bad = S.CSR.from_rows([[(0, 1)], [(3, 1)]], 4, prime=p)
        bad.j[1] = 4
        assert fn(Dev._need(), bad.data, C.byref(out), okp) == -1 and "column index" in S._abi.last_error() and untouched()
        assert fn(Dev._need(), None, C.byref(out), okp) == -1 and "NULL matrix" in S._abi.last_error() and untouched()
        with pytest.raises(ValueError):
            Dev.solve(S.CSR.from_rows([[]], 5, prime=p))
        with pytest.raises(S.SpasmError, match="prime"):
            Dev.solve(S.CSR.from_rows([[]], 4, prime=7))
        X, ok = Dev.solve(S.CSR.from_rows([[(0, 2), (1, 4)], [(3, 0)], [(3, 1)], []], 4, prime=p))
        assert ok.tolist() == [True, True, False, True] and X.rows() == [[(0, 2)], [], [], []] and S._abi.last_error() == ""


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. against gesv where the solution is unique
# ---------------------------------------------------------------------------------------------------------------------------------
def test_full_row_rank_systems_agree_with_gesv(S):
    rng = np.random.default_rng(8)
    As, Bs = [], []
    for t in range(20):
        p = [127, 65521, 4294967291][t % 3]
        n = int(rng.integers(2, 30))
        m = n + int(rng.integers(0, 12))
        A = rng.integers(0, p, size=(n, m)).astype(object) * (rng.random((n, m)) < 0.5)
        for i in range(n):
            A[i, i] = 1 + int(rng.integers(0, p - 1))
            A[i, :i] = 0  # upper triangular with a non-zero diagonal: full row rank
        A = A[rng.permutation(n)][:, rng.permutation(m)]
        Y = rng.integers(0, p, size=(5, n)).astype(object)
        As.append(make_csr(S, A % p, p, rng, False))
        Bs.append(make_csr(S, (Y @ A) % p, p, rng, False))
    X, ok = S.solve_batch(As, Bs)
    assert S.solve_stats()["general_path"] == 0
    for A, B, x, o in zip(As, Bs, X, ok):
        Xg, okg = S.gesv(S.echelonize(A, L=True), B)
        assert o.all(), o
        assert okg.all(), okg
        # densified: gesv leaves the entries of a row in pivot order and may store a zero
        p, dt = A.prime, object if A.prime >= 2 ** 31 else np.int64
        assert x.shape == Xg.shape == (B.n, A.n)
        assert np.array_equal(dense(x.rows(), B.n, A.n, dt) % p, dense(Xg.rows(), B.n, A.n, dt) % p)
