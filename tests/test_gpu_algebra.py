"""Exact matrix algebra on the device: A B, a A + b B, submatrices (spasm_amd_dcsr_*, spasm_amd_csr_mul / _lincomb, the operators of
CSR and DeviceCSR).  Every expected value comes from exact integers computed independently of the library: values reduced to
[0, p), products taken in uint64 and reduced per term (p^2 < 2^64), summed per (row, column) key with np.add.at (terms * p < 2^63
at these sizes), zeros dropped, keys sorted."""
import gc

import numpy as np
import pytest

from conftest import LM

pytestmark = pytest.mark.gpu

PRIMES = [3, 127, 42013, 65521, 2**31 - 1, 0xFFFFFFFB]


def csr_arrays(A):
    k = int(A.p[A.n])
    return np.asarray(A.p, dtype=np.int64).copy(), A.j[:k].astype(np.int64), A.x[:k].astype(np.int64)


def canon(n, m, rows, cols, vals, p):
    """canonical CSR arrays of the matrix sum of the terms (rows, cols, vals), vals in [0, p); also the number of distinct keys"""
    key = rows.astype(np.int64) * max(m, 1) + cols.astype(np.int64)
    uk, inv = np.unique(key, return_inverse=True)
    distinct = len(uk)
    acc = np.zeros(len(uk), dtype=np.int64)
    np.add.at(acc, inv, vals.astype(np.int64))
    acc %= p
    keep = acc != 0
    uk, acc = uk[keep], acc[keep]
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(ptr, uk // max(m, 1) + 1, 1)
    ptr = np.cumsum(ptr)
    return ptr, (uk % max(m, 1)).astype(np.int32), np.where(2 * acc > p, acc - p, acc).astype(np.int32), distinct


def ref_mul(A, B):
    p = A.prime
    pa, ja, xa = csr_arrays(A)
    pb, jb, xb = csr_arrays(B)
    row_a = np.repeat(np.arange(A.n), np.diff(pa))
    cnt = np.diff(pb)[ja] if len(ja) else np.zeros(0, np.int64)
    ia = np.repeat(np.arange(len(ja)), cnt)
    ib = np.repeat(pb[ja] if len(ja) else np.zeros(0, np.int64), cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    prod = ((xa[ia] % p).astype(np.uint64) * (xb[ib] % p).astype(np.uint64)) % np.uint64(p)
    return canon(A.n, B.m, row_a[ia], jb[ib], prod, p)


def ref_lincomb(a, A, b, B):
    p = A.prime
    rows, cols, vals = [], [], []
    for s, M in ((a, A), (b, B)):
        if M is None:
            continue
        pm, jm, xm = csr_arrays(M)
        rows.append(np.repeat(np.arange(M.n), np.diff(pm)))
        cols.append(jm)
        vals.append((((xm % p).astype(np.uint64) * np.uint64(s % p)) % np.uint64(p)).astype(np.int64))
    return canon(A.n, A.m, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), p)


def same(C, want, what=""):
    ptr, j, x = want[:3]
    k = int(ptr[-1])
    assert S_nnz(C) == k and C.nzmax == k, (what, S_nnz(C), C.nzmax, k)
    assert np.array_equal(np.asarray(C.p), ptr), what
    assert np.array_equal(C.j[:k], j) and np.array_equal(C.x[:k], x), what


def S_nnz(C):
    return int(C.p[C.n])


def messy(S, n, m, density, p, rng, reduced=False):
    """n x m: unsorted rows, every fifth row empty, duplicate columns, explicit zeros, any int32 as a value"""
    rows = []
    for i in range(n):
        cnt = 0 if (i % 5 == 0 or m == 0) else rng.binomial(m, density) + int(rng.integers(0, 3))
        rows.append(rng.integers(0, m, size=cnt) if cnt else np.zeros(0, dtype=np.int64))  # with replacement: duplicates
    ptr = np.zeros(n + 1, dtype=np.int64)
    if n:
        ptr[1:] = np.cumsum([len(r) for r in rows])
    j = np.concatenate(rows).astype(np.int32) if n else np.zeros(0, np.int32)
    x = rng.integers(-(2**31), 2**31, size=len(j), dtype=np.int64)
    x[rng.random(len(j)) < 0.1] = 0
    if reduced:
        x = S.balanced(x, p).astype(np.int64)
    return S.CSR.from_arrays(n, m, ptr, j, x.astype(np.int32), prime=p)


SHAPES = [((40, 40), (40, 40)), ((17, 300), (300, 9)), ((300, 17), (17, 300)), ((0, 9), (9, 4)), ((5, 0), (0, 7)), ((0, 0), (0, 0))]


@pytest.mark.parametrize("p", PRIMES)
@pytest.mark.parametrize("shapes", SHAPES)
def test_products_entry_for_entry(S, p, shapes):
    (n, k), (k2, m) = shapes
    rng = np.random.default_rng(p % 100003 + 13 * n + m)
    A = messy(S, n, k, 0.3 if p == 3 else 0.15, p, rng)
    B = messy(S, k2, m, 0.3 if p == 3 else 0.15, p, rng)
    want = ref_mul(A, B)
    C = A @ B
    assert C.shape == (n, m) and C.prime == p
    same(C, want, (p, shapes))
    if p == 3 and n >= 17 and m >= 9:
        assert int(want[0][-1]) < want[3], "no sum cancels: the case does not exercise the dropping of zeros"
    with S.DeviceCSR(A) as a, S.DeviceCSR(B) as b:
        c = a @ b
        assert c.shape == (n, m) and c.nnz == int(want[0][-1]) and c.prime == p
        same(c.download(), want)
        c.close()


def all_paths_pair(S, p):
    """rows of A with bounds 1, 30, ~100, 1000, 3000, 10^4, combinations of them, a full row of m = 200 000 columns (twice)"""
    rng = np.random.default_rng(99)
    m = 200_000
    lens = [1, 30, 100, 1000, 3000, 10_000, m, 0]
    cols = [rng.permutation(m)[:l] if l < m else rng.permutation(m) for l in lens]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    j = np.concatenate(cols).astype(np.int32)
    B = S.CSR.from_arrays(len(lens), m, ptr, j, S.balanced(rng.integers(1, p, size=len(j)), p), prime=p)
    arows = [[0], [1], [2], [3], [4], [5], [6], [7], [], [0, 1, 0], [1, 2, 3], [3, 3], [2, 4, 5], [6, 6], [5, 6, 1], [7, 7, 0], [4, 4, 4, 4], [3] * 9]
    aptr = np.concatenate([[0], np.cumsum([len(r) for r in arows])]).astype(np.int64)
    aj = np.concatenate([np.array(r, dtype=np.int32) for r in arows])
    A = S.CSR.from_arrays(len(arows), len(lens), aptr, aj, S.balanced(rng.integers(1, p, size=len(aj)), p), prime=p)
    return A, B


@pytest.mark.parametrize("p", [65521, 0xFFFFFFFB])
def test_every_path_is_taken_and_agrees(S, p):
    A, B = all_paths_pair(S, p)
    want = ref_mul(A, B)
    with S.DeviceCSR(A) as a, S.DeviceCSR(B) as b:
        c = a @ b
        st = c.stats()
        print("stats", p, st)
        assert st["rows_tiny"] > 0 and st["rows_hash"] > 0 and st["rows_global"] > 0, st
        assert st["flops"] == sum(int(np.diff(B.p)[B_row]) for B_row in A.j[: int(A.p[A.n])]) and st["entries"] == int(want[0][-1])
        same(c.download(), want)


def test_determinism_three_runs(S):
    A, B = all_paths_pair(S, 65521)
    outs = []
    for _ in range(3):
        C = A @ B
        outs.append((np.asarray(C.p).tobytes(), C.j[: S_nnz(C)].tobytes(), C.x[: S_nnz(C)].tobytes()))
    assert outs[0] == outs[1] == outs[2]


def test_chunked_rows_give_the_same_matrix(S, monkeypatch):
    p = 42013
    rng = np.random.default_rng(8)
    A = messy(S, 3000, 2000, 0.01, p, rng)
    B = messy(S, 2000, 2500, 0.01, p, rng)
    want = ref_mul(A, B)
    with S.DeviceCSR(A) as a, S.DeviceCSR(B) as b:
        one = a @ b
        assert one.stats()["chunks"] == 1
        monkeypatch.setenv("SPASM_AMD_SPGEMM_SCRATCH_MB", "1")
        many = a @ b
        monkeypatch.delenv("SPASM_AMD_SPGEMM_SCRATCH_MB")
        assert many.stats()["chunks"] > 1, many.stats()
        assert many.equals(one)
        same(many.download(), want)
        # a row that does not fit the budget at all is an error with a text, not a crash
        monkeypatch.setenv("SPASM_AMD_SPGEMM_SCRATCH_MB", "0.0001")
        with pytest.raises(S.SpasmError, match="scratch"):
            a @ b
        monkeypatch.delenv("SPASM_AMD_SPGEMM_SCRATCH_MB")
        assert (a @ b).equals(one)


@pytest.mark.parametrize("p", [65521, 0xFFFFFFFB])
def test_accumulator_bound_long_inner_dimension(S, p):
    """4 194 304 terms of halfp * halfp on one output entry: a row whose BOUND is 2^22 although it has one column"""
    L = 4_194_304
    h = p // 2
    row = S.CSR.from_arrays(1, L, np.array([0, L]), np.arange(L, dtype=np.int32), np.full(L, h, dtype=np.int32), prime=p)
    col = S.CSR.from_arrays(L, 1, np.arange(L + 1), np.zeros(L, dtype=np.int32), np.full(L, h, dtype=np.int32), prime=p)
    with S.DeviceCSR(row) as a, S.DeviceCSR(col) as b:
        c = a @ b
        assert c.stats()["rows_global"] == 1 and c.stats()["max_bound"] == L
        C = c.download()
    assert C.shape == (1, 1) and S_nnz(C) == 1 and C.j[0] == 0
    assert int(C.x[0]) == S.ZZp(p, L * h * h)
    # the twin: few terms per entry, many entries
    Lp = 3000
    colp = S.CSR.from_arrays(Lp, 1, np.arange(Lp + 1), np.zeros(Lp, dtype=np.int32), np.full(Lp, h, dtype=np.int32), prime=p)
    rowp = S.CSR.from_arrays(1, Lp, np.array([0, Lp]), np.arange(Lp, dtype=np.int32), np.full(Lp, h, dtype=np.int32), prime=p)
    D = colp @ rowp
    assert D.shape == (Lp, Lp) and S_nnz(D) == Lp * Lp == D.nzmax
    assert np.array_equal(np.asarray(D.p), np.arange(Lp + 1, dtype=np.int64) * Lp)
    assert np.array_equal(D.j[: Lp * Lp].reshape(Lp, Lp), np.broadcast_to(np.arange(Lp, dtype=np.int32), (Lp, Lp)))
    assert np.all(D.x[: Lp * Lp] == S.ZZp(p, h * h))


@pytest.mark.parametrize("p", PRIMES)
def test_linear_combinations(S, p):
    rng = np.random.default_rng(p % 9973)
    n, m = 120, 90
    A = messy(S, n, m, 0.1, p, rng)
    B = messy(S, n, m, 0.1, p, rng)
    scalars = [0, 1, -1, p, 2**32 + 12345, -(2**40) - 7, 2**63 - 1, -(2**63)] + [int(v) for v in rng.integers(-(2**62), 2**62, size=3)]
    with S.DeviceCSR(A) as a, S.DeviceCSR(B) as b:
        for t, sa in enumerate(scalars):
            sb = scalars[(3 * t + 1) % len(scalars)]
            same(a.lincomb(sa, sb, b).download(), ref_lincomb(sa, A, sb, B), (p, sa, sb))
        same((a + b).download(), ref_lincomb(1, A, 1, B))
        same((a - b).download(), ref_lincomb(1, A, -1, B))
        same((7 * a).download(), ref_lincomb(7, A, 0, None))
        assert (a - a).nnz == 0 and (a * p).nnz == 0 and (0 * a).nnz == 0
        # the canonical form of a matrix that is not canonical
        same(a.lincomb(1).download(), ref_lincomb(1, A, 0, None))
        assert a.lincomb(1).equals(a) and a.equals(a.lincomb(1)) and not a.equals(b)
        assert (-a).equals((p - 1) * a) and (-a).equals(a * (p - 1))
    same(A + B, ref_lincomb(1, A, 1, B))
    same(A - B, ref_lincomb(1, A, -1, B))
    same(-A, ref_lincomb(-1, A, 0, None))
    same((2**32 + 5) * A, ref_lincomb(2**32 + 5, A, 0, None))
    assert S_nnz(A - A) == 0
    assert (-A).equals((p - 1) * A) and A.equals(A + (A - A)) and not A.equals(B)


@pytest.mark.parametrize("p", [127, 0xFFFFFFFB])
def test_submatrix_on_the_device_equals_the_host(S, p):
    rng = np.random.default_rng(p % 1000)
    n, m = 11, 30
    A = messy(S, n, m, 0.3, p, rng)
    ranges = [((0, 0), (0, 0)), ((3, 3), (0, 7)), ((0, 9), (4, 4)), ((2, 11), (5, 23)), ((0, 1), (0, 1)), ((7, 8), (29, 30)), ((0, n), (0, m))]
    with S.DeviceCSR(A) as a:
        for (r0, r1), (c0, c1) in ranges:
            d = a[r0:r1, c0:c1]
            assert d.shape == (r1 - r0, c1 - c0)
            H = S.submatrix(A, range(r0, r1), range(c0, c1))  # stored order, duplicates and zeros kept
            same(d.download(), ref_lincomb(1, H, 0, None), (r0, r1, c0, c1))
        with pytest.raises(ValueError):
            a[::2, :]
        lib = S._abi.lib()
        assert not lib.spasm_amd_dcsr_submatrix(a._h, 0, n + 1, 0, m) and "range" in S._abi.last_error()
        assert not lib.spasm_amd_dcsr_submatrix(a._h, 5, 2, 0, m) and "range" in S._abi.last_error()
    # a big one through every class of rows
    Abig, Bbig = all_paths_pair(S, 65521)
    with S.DeviceCSR(Bbig) as b:
        H = S.submatrix(Bbig, range(1, 8), range(1000, 150_000))
        same(b[1:8, 1000:150_000].download(), ref_lincomb(1, H, 0, None))


def test_errors_leave_the_text_and_the_operands(S):
    A = messy(S, 6, 7, 0.3, 127, np.random.default_rng(1), reduced=True)
    B = messy(S, 6, 7, 0.3, 127, np.random.default_rng(2), reduced=True)
    B2 = messy(S, 7, 6, 0.3, 65521, np.random.default_rng(3), reduced=True)
    lib = S._abi.lib()
    before = csr_arrays(A)
    assert not lib.spasm_amd_csr_mul(A.data, B.data) and "dimension" in S._abi.last_error()
    assert not lib.spasm_amd_csr_mul(A.data, B2.data) and "prime" in S._abi.last_error()
    assert not lib.spasm_amd_csr_lincomb(1, A.data, 1, B2.data) and S._abi.last_error() != ""
    assert not lib.spasm_amd_csr_mul(None, B.data) and S._abi.last_error() != ""
    P = S.submatrix(A, range(0, 6), range(0, 7), with_values=False)
    assert not lib.spasm_amd_dcsr_upload(P.data) and "values" in S._abi.last_error()
    bad = S.CSR.from_arrays(1, 3, np.array([0, 2]), np.array([1, 3], dtype=np.int32), np.array([1, 1], dtype=np.int32), prime=127)  # column 3 of 3
    assert not lib.spasm_amd_dcsr_upload(bad.data) and "column" in S._abi.last_error()
    with S.DeviceCSR(A) as a, S.DeviceCSR(B2) as b2:
        with pytest.raises(ValueError):
            a @ b2
        assert not lib.spasm_amd_dcsr_mul(a._h, b2._h) and "prime" in S._abi.last_error()
        assert lib.spasm_amd_dcsr_equal(a._h, b2._h) == 0
        a + a
        assert S._abi.last_error() == ""
    assert all(np.array_equal(u, v) for u, v in zip(before, csr_arrays(A)))


def test_lu_equals_a(S):
    p = 42013
    rng = np.random.default_rng(21)
    n, m, r = 2000, 1500, 900
    # rank at most r: rows are sparse combinations of r sparse rows
    base = messy(S, r, m, 0.004, p, rng, reduced=True)
    comb = messy(S, n, r, 0.003, p, rng, reduced=True)
    A = comb @ base
    fact = S.echelonize(A, L=True, **LM)
    assert fact.r < m
    LU = fact.L @ fact.U
    assert LU.shape == A.shape and LU.equals(A) and A.equals(LU)
    assert S_nnz(LU - A) == 0


def test_kernel_basis_as_a_matrix_identity(S):
    p = 42013
    B = S.synth_csr(0, 9_850, 10_000, density=1e-3, prime=p, seed=0x5A5A0007)
    ptr, j, v = csr_arrays(B)
    A = S.CSR.from_arrays(10_000, 10_000, np.concatenate([ptr, np.full(150, ptr[-1])]), j.astype(np.int32), v.astype(np.int32), prime=p)
    K = S.kernel(S.echelonize(A))
    assert K.n >= 150 and K.m == A.m
    Z = A @ S.transpose(K)
    assert Z.shape == (A.n, K.n) and S_nnz(Z) == 0  # every entry is a sum that cancels
    assert ref_mul(A, S.transpose(K))[3] > 0        # .. and there were sums


def test_transpose_and_associativity(S):
    p = 65521
    rng = np.random.default_rng(5)
    A = messy(S, 300, 200, 0.05, p, rng)
    B = messy(S, 200, 250, 0.05, p, rng)
    Cm = messy(S, 250, 180, 0.05, p, rng)
    assert S.transpose(A @ B).equals(S.transpose(B) @ S.transpose(A))
    with S.DeviceCSR(A) as a, S.DeviceCSR(B) as b, S.DeviceCSR(Cm) as c:
        left, right = (a @ b) @ c, a @ (b @ c)
        assert left.equals(right) and left.nnz == right.nnz > 0
        same(left.download(), ref_mul(A @ B, Cm))


def test_handle_lifetime(S):
    p = 127
    rng = np.random.default_rng(6)
    A = messy(S, 50, 40, 0.1, p, rng)
    B = messy(S, 40, 30, 0.1, p, rng)
    want = ref_mul(A, B)
    a, b = S.DeviceCSR(A), S.DeviceCSR(B)
    del A, B
    gc.collect()
    c = a @ b
    a.close()
    a.close()
    b.close()
    same(c.download(), want)  # a result does not depend on its operands
    for call in (lambda: a @ c, lambda: c @ a, lambda: a.download(), lambda: a.stats(), lambda: -a, lambda: a[0:1, 0:1], lambda: a.equals(c), lambda: c.equals(a)):
        with pytest.raises(S.SpasmError):
            call()
    c.close()
    c.close()


def test_config3_squared_full_size(S):
    """A = config 3 (10^6 x 10^6, 20 entries per row), C = A A on resident handles: about 4 * 10^8 products"""
    import torch

    p = 65521
    small = S.synth_csr(1, 100_000, 100_000, row_nnz=20, prime=p, seed=0x5A5A0003)
    with S.DeviceCSR(small) as d:
        e = d @ d
        st = e.stats()
        need = 10 * (st["scratch_bytes"] + 2 * 8 * st["entries"] + 8 * small.nzmax)  # scratch + result + its unpacked copy + A
        e.close()
    free = torch.cuda.mem_get_info()[0]
    if free < 3 * need:  # (the scratch budget is a third of the free memory)
        pytest.skip(f"free device memory {free / 2**30:.1f} GiB, the full-size product needs about {3 * need / 2**30:.1f} GiB")
    A = S.synth_csr(1, 1_000_000, 1_000_000, row_nnz=20, prime=p, seed=0x5A5A0003)
    with S.DeviceCSR(A) as a:
        c = a @ a
        st = c.stats()
        print("config 3 squared:", st)
        assert st["flops"] == 400_000_000 and st["entries"] == c.nnz
        C = c.download()
        c.close()
    k = S_nnz(C)
    assert C.shape == (A.n, A.m) and C.nzmax == k
    # (b) canonical form
    ptr, j, x = np.asarray(C.p), C.j[:k], C.x[:k]
    assert ptr[0] == 0 and np.all(np.diff(ptr) >= 0)
    inner = np.ones(k, dtype=bool)
    inner[ptr[:-1][np.diff(ptr) > 0]] = False  # first entry of each row
    assert np.all(np.diff(j.astype(np.int64))[inner[1:]] > 0), "columns must ascend inside every row"
    assert j.min() >= 0 and j.max() < A.m
    assert np.all(x != 0) and x.min() >= -(p // 2) and x.max() <= p // 2
    # (a) random projections through the exact SpMV
    rng = np.random.default_rng(17)
    with S.SpMV(A) as opa, S.SpMV(C) as opc:
        X = S.balanced(rng.integers(0, p, size=(A.n, 4)), p)
        assert np.array_equal(opc.apply(X, trans=True), opa.apply(opa.apply(X, trans=True), trans=True))
    # (c) 1000 rows entry for entry
    pick = np.sort(rng.choice(A.n, size=1000, replace=False))
    pa, ja, xa = csr_arrays(A)
    idx = np.concatenate([np.arange(pa[i], pa[i + 1]) for i in pick])
    sub = S.CSR.from_arrays(1000, A.m, np.concatenate([[0], np.cumsum(pa[pick + 1] - pa[pick])]), ja[idx].astype(np.int32), xa[idx].astype(np.int32), prime=p)
    wp, wj, wx, _ = ref_mul(sub, A)
    for t, i in enumerate(pick):
        lo, hi = int(ptr[i]), int(ptr[i + 1])
        assert hi - lo == wp[t + 1] - wp[t] and np.array_equal(j[lo:hi], wj[wp[t]:wp[t + 1]]) and np.array_equal(x[lo:hi], wx[wp[t]:wp[t + 1]]), i
