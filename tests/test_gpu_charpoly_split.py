"""GPU tests of the characteristic polynomial by components: the index split (spasm_amd_blocks_create_index; csrc/blocks.hpp), the
product tree (spasm_amd_poly_product; csrc/polyprod.hpp) and spasm_amd_blocks_charpoly / _charpoly_factors / _charpoly_split.

Every expected value is known by construction or from exact Python integers: the device maps are compared with the pure-Python
union-find of Block.from_csr(A, index=True); products with the schoolbook convolution in Python integers; characteristic
polynomials with the product of the polynomials whose companion matrices were put on the diagonal."""
import ctypes as C
from math import comb

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P16, P31, P32 = 65521, 2147483647, 4294967291
PRIMES = (3, 5, 127, P16, P31, P32)
SENTINEL = 0x5A5A5A5A
PP_WAVE = 64   # csrc/polyprod.hpp: a shorter factor of at least this many words is walked by a wave per output word
I32P = C.POINTER(C.c_int32)


def bal(v, p):
    v = np.array([int(x) % p for x in v], dtype=np.int64)
    return np.where(v > p // 2, v - p, v).astype(np.int32)


def polymul(a, b, p):
    """schoolbook convolution in Python integers, residues in [0, p)"""
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        x = int(x)
        if x:
            for j, y in enumerate(b):
                out[i + j] += x * int(y)
    return [v % p for v in out]


def product(polys, p):
    out = [1]
    for f in polys:
        out = polymul(out, f, p)
    return out


def check(got, want, p):
    want = bal(want, p)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]


def random_rows(rng, n, per_row, p=127):
    rows = []
    for _ in range(n):
        k = int(rng.integers(0, per_row + 1))
        rows.append([(int(c), int(rng.integers(1, p))) for c in sorted(set(rng.integers(0, n, size=k).tolist()))])
    return rows


def companion_rows(coef, p):
    """rows of the companion matrix of the monic coef (low degree first): ones on the subdiagonal, -coef in the last column (zeros
    are not stored; the subdiagonal alone keeps the indices of the block in one component)"""
    n = len(coef) - 1
    rows = []
    for i in range(n):
        r = [(i - 1, 1)] if i > 0 else []
        v = -int(coef[i]) % p
        if v:
            r.append((n - 1, v))
        rows.append(r)
    return rows


def random_monic(rng, n, p):
    return [int(v) for v in rng.integers(0, p, size=n)] + [1]


def block_diagonal(S, polys, p, rng):
    """(A, D, q): the companion matrices of polys on the diagonal, scrambled by a random simultaneous permutation q on the device
    (D = DeviceCSR.permute(q, q), A its download); index i of A is index q[i] of the block-diagonal matrix"""
    rows, base = [], 0
    for f in polys:
        for r in companion_rows(f, p):
            rows.append([(base + c, v) for c, v in r])
        base += len(f) - 1
    q = rng.permutation(base).astype(np.int32)
    with S.DeviceCSR(S.CSR.from_rows(rows, base, prime=p)) as D0:
        D = D0.permute(q, q)
    return D.download(), D, q


def maps_equal(S, D, B):
    r2b, c2b, b2r, b2c = D.block_maps()
    assert r2b == B.row2block and c2b == B.col2block and b2r == B.block2row and b2c == B.block2col
    assert len(D) == len(B)
    for b, X in enumerate(B.blocks):
        Y = D.fetch(b)
        assert Y.shape == X.shape
        assert np.array_equal(Y.p[: Y.n + 1], X.p[: X.n + 1])
        nz = int(X.p[X.n])
        assert np.array_equal(Y.j[:nz], X.j[:nz]) and np.array_equal(Y.x[:nz], X.x[:nz])


def index_properties(D):
    mp = D.maps()
    assert np.array_equal(mp["row_pos"], mp["col_pos"]) and np.array_equal(mp["row_block"], mp["col_block"])
    assert np.array_equal(mp["block_rows"], mp["block_cols"]) and np.array_equal(mp["row_start"], mp["col_start"])
    rows, cols, _ = D.shapes()
    assert np.array_equal(rows, cols) and (len(rows) == 0 or rows.min() >= 1)
    first = mp["block_rows"][mp["row_start"][:-1]]
    assert np.all(np.diff(first) > 0)   # blocks ascend by smallest index
    return mp


# ---------------------------------------------------------------------------------------------
# the index split
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, per_row", [(1, 1), (2, 1), (50, 1), (3000, 1)])
def test_device_index_maps_equal_the_host_union_find(S, n, per_row):
    rng = np.random.default_rng(1000 + n)
    A = S.CSR.from_rows(random_rows(rng, n, per_row), n, prime=127)
    B = S.Block.from_csr(A, index=True)
    with S.DeviceBlocks(A, index=True) as D, S.DeviceBlocks(A, index=True) as D2, S.DeviceBlocks(A) as free:
        assert D.index is True and free.index is False
        maps_equal(S, D, B)
        mp, mp2 = index_properties(D), D2.maps()
        assert all(mp[k].tobytes() == mp2[k].tobytes() for k in mp)   # two handles of one matrix
        for b in range(len(D)):
            X, Y = D.fetch(b), D2.fetch(b)
            assert X.j[: S.nnz(X)].tobytes() == Y.j[: S.nnz(Y)].tobytes() and X.x[: S.nnz(X)].tobytes() == Y.x[: S.nnz(Y)].tobytes()
        assert sum(D.rank()) == sum(free.rank())
        assert D.det() == S.det(A)
    with S.DeviceCSR(A) as R, S.DeviceBlocks(R, index=True) as D:
        assert D.index is True
        maps_equal(S, D, B)
    assert S.Block.from_csr(A, device=True, index=True).block2row == B.block2row


def test_index_split_of_special_graphs(S):
    p = 127
    # one row longer than BLK_LONG (512): the workgroup walk of the long rows
    rng = np.random.default_rng(5)
    rows = random_rows(rng, 700, 1)
    rows[3] = [(c, 1 + c % 100) for c in range(40, 640)]
    # joined only through the tie: row i and column i lie in different components of the free graph
    tie = [[(1, 5)], [(2, 6)], []]
    # explicit zeros join
    zeros = [[(1, 0)], [(1, 5)], [], [(3, 7)], [(2, 0)]]
    cyc = [[(1, 1)], [(2, 1)], [(0, 1)]]
    for rws, want in ((rows, None), (tie, [[0, 1, 2]]), (zeros, [[0, 1], [2, 4], [3]]), (cyc, [[0, 1, 2]])):
        A = S.CSR.from_rows(rws, len(rws), prime=p)
        B = S.Block.from_csr(A, index=True)
        if want is not None:
            assert B.block2row == want
        with S.DeviceBlocks(A, index=True) as D:
            maps_equal(S, D, B)
            index_properties(D)
            assert D.det() == S.det(A)
    with S.DeviceBlocks(S.CSR.from_rows(tie, 3, prime=p)) as free:
        assert len(free) == 4 and free.index is False   # {r0, c1}, {r1, c2}, {r2}, {c0}


def test_the_trap_three_cycle(S):
    A = S.CSR.from_rows([[(1, 1)], [(2, 1)], [(0, 1)]], 3, prime=127)
    with S.DeviceBlocks(A, index=True) as D:
        assert len(D) == 1
        check(D.charpoly(), [-1, 0, 0, 1], 127)
        assert [f.tolist() for f in D.charpoly_factors()] == [[-1, 0, 0, 1]]
    check(S.charpoly(A, split=True), [-1, 0, 0, 1], 127)
    with S.DeviceBlocks(A) as free:
        assert len(free) == 3
        lib = S._abi.lib()
        buf = (C.c_int32 * 8)(*([SENTINEL] * 8))
        for fn, who in ((lib.spasm_amd_blocks_charpoly, "spasm_amd_blocks_charpoly"), (lib.spasm_amd_blocks_charpoly_factors, "spasm_amd_blocks_charpoly_factors")):
            assert fn(free._need(), C.cast(buf, I32P)) == -1
            assert S._abi.last_error() == who + ": the handle is not an index split (spasm_amd_blocks_create_index)"
        assert all(v == SENTINEL for v in buf)
        with pytest.raises(S.SpasmError, match="not an index split"):
            free.charpoly()
        with pytest.raises(S.SpasmError, match="not an index split"):
            S.blocks.charpoly(free)


# ---------------------------------------------------------------------------------------------
# the product kernel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 3, 5, 8, 9])
def test_product_counts_with_odd_carries(S, count):
    rng = np.random.default_rng(count)
    for p in (127, P32):
        polys = [[int(v) for v in rng.integers(0, p, size=int(rng.integers(1, 6)))] for _ in range(count)]
        check(S.poly_product([bal(f, p) for f in polys], p), product(polys, p), p)


@pytest.mark.parametrize("short", [1, 2, PP_WAVE - 1, PP_WAVE, PP_WAVE + 1])
def test_product_walking_shapes_and_their_boundary(S, short):
    rng = np.random.default_rng(short)
    long_ = 2 * PP_WAVE + 3
    for p in (5, P16, P32):
        u = [int(v) for v in rng.integers(0, p, size=short)]
        v = [int(x) for x in rng.integers(0, p, size=long_)]
        want = polymul(u, v, p)
        check(S.poly_product([bal(u, p), bal(v, p)], p), want, p)
        check(S.poly_product([bal(v, p), bal(u, p)], p), want, p)
        # a second level on top: (u * v) * (v * u) has a shorter factor of short + long_ - 1 >= PP_WAVE words
        check(S.poly_product([bal(u, p), bal(v, p), bal(v, p), bal(u, p)], p), polymul(want, want, p), p)


@pytest.mark.parametrize("p", PRIMES)
def test_product_of_extreme_coefficients(S, p):
    h = (p - 1) // 2
    for la, lb in ((3, 2), (PP_WAVE - 1, 2 * PP_WAVE + 3), (PP_WAVE + 1, 2 * PP_WAVE + 3)):
        for sa, sb in ((1, 1), (1, -1), (-1, -1)):
            u, v = [sa * h] * la, [sb * h] * lb
            got = S.poly_product([np.array(u, dtype=np.int32), np.array(v, dtype=np.int32)], p)
            check(got, polymul([x % p for x in u], [x % p for x in v], p), p)
    alt = [h if i % 2 else -h for i in range(2 * PP_WAVE + 3)]
    check(S.poly_product([np.array(alt, dtype=np.int32)] * 3, p), product([[x % p for x in alt]] * 3, p), p)


def test_product_reduces_its_input_and_keeps_zero_factors(S):
    for p in (3, 127, P32):
        raw = [[2**31 - 1, -(2**31), 7], [-5, 2**31 - 2], [123456789, -987654321, 0]]   # unreduced, negative, a zero leading word
        check(S.poly_product(raw, p), product([[x % p for x in f] for f in raw], p), p)
        check(S.poly_product([raw[0]], p), [x % p for x in raw[0]], p)   # one factor: reduced, no level
        zero_mod_p = [p, -p, 2 * p] if p < 2**30 else [0, 0, 0]
        got = S.poly_product([raw[0], [0, 0], raw[1], zero_mod_p], p)   # a zero polynomial, and one that is zero mod p
        assert got.shape == (3 + 2 + 2 + 3 - 3,) and not got.any()


def test_product_of_ten_thousand_linear_factors(S):
    p, n = P16, 10000
    rng = np.random.default_rng(77)
    roots = rng.integers(0, p, size=n)
    polys = [np.array([-int(r) % p, 1], dtype=np.int64) for r in roots]
    # the same convolution, pairwise, in int64: at most 5001 terms below p^2 < 2^32 each, so every sum stays below 2^45
    assert [int(v) for v in np.convolve(polys[0], polys[1]) % p] == polymul(polys[0], polys[1], p)
    level = polys
    while len(level) > 1:
        level = [np.convolve(level[k], level[k + 1]) % p if k + 1 < len(level) else level[k] for k in range(0, len(level), 2)]
    want = level[0]   # coefficient n - k is (-1)^k e_k(roots)
    assert want[n] == 1 and int(want[n - 1]) == -int(roots.sum()) % p
    arg = [bal(f, p) for f in polys]
    got = S.poly_product(arg, p)
    check(got, want, p)
    assert S.poly_product(arg, p).tobytes() == got.tobytes()


# ---------------------------------------------------------------------------------------------
# the characteristic polynomial by blocks
# ---------------------------------------------------------------------------------------------
SIZES = (1, 2, 31, 33, 64, 111, 181, 182, 600)   # the four LDS classes, and the global path


@pytest.fixture(scope="module")
def companions(S):
    p = P16
    rng = np.random.default_rng(2024)
    polys = [random_monic(rng, n, p) for n in SIZES]
    A, D, q = block_diagonal(S, polys, p, rng)
    yield p, polys, A, D, q
    D.close()


def test_charpoly_by_blocks_of_companion_matrices(S, companions):
    p, polys, A, D, q = companions
    n = sum(SIZES)
    assert A.n == n == 1205
    want = product(polys, p)
    check(S.charpoly(A, split=True), want, p)
    check(S.charpoly(D, split=True), want, p)
    with pytest.raises(S.SpasmError, match=r"characteristic polynomial limited to n <= 1024 \(n = 1205\)"):
        S.charpoly(A)
    B = S.Block.from_csr(A, index=True)
    check(S.blocks.charpoly(B), want, p)
    with S.DeviceBlocks(D, index=True) as X:
        assert len(X) == len(SIZES)
        check(X.charpoly(), want, p)
        check(S.blocks.charpoly(X), want, p)
        st = S.charpoly_split_stats()
        assert (st["blocks"], st["lds_path"], st["global_path"], st["product_levels"]) == (9, 7, 2, 4)
        assert 2 <= st["launches"] <= 5 and st["spare"] == 0
        # the factors: block b of the handle is the companion block that holds index q[block_rows[first of b]]
        factors, mp = X.charpoly_factors(), X.maps()
        starts = np.concatenate(([0], np.cumsum(SIZES)))
        for b, f in enumerate(factors):
            orig = int(q[mp["block_rows"][mp["row_start"][b]]])
            k = int(np.searchsorted(starts, orig, side="right") - 1)
            check(f, polys[k], p)


def test_counters_of_a_call_with_both_paths_and_three_levels(S):
    p = 127
    rng = np.random.default_rng(9)
    polys = [random_monic(rng, n, p) for n in (3, 5, 200, 2, 7)]
    A, D, _ = block_diagonal(S, polys, p, rng)
    D.close()
    check(S.charpoly(A, split=True), product(polys, p), p)
    st = S.charpoly_split_stats()
    assert (st["blocks"], st["lds_path"], st["global_path"], st["product_levels"], st["spare"]) == (5, 4, 1, 3, 0)
    assert 2 <= st["launches"] <= 5 and st["charpoly_device_us"] >= 0 and st["product_device_us"] >= 0


def test_total_over_the_limit_made_of_small_blocks(S):
    p = P31
    rng = np.random.default_rng(31)
    polys = [random_monic(rng, n, p) for n in (200, 190, 180, 170, 160, 150, 140, 130, 100, 80)]
    A, D, _ = block_diagonal(S, polys, p, rng)
    D.close()
    assert A.n == 1500
    with pytest.raises(S.SpasmError, match=r"^spasm_amd_charpoly: characteristic polynomial limited to n <= 1024 \(n = 1500\)$"):
        S.charpoly(A)
    check(S.charpoly(A, split=True), product(polys, p), p)


@pytest.mark.parametrize("p", PRIMES)
def test_split_equals_the_whole_matrix_byte_for_byte(S, p):
    rng = np.random.default_rng(p % 1000)
    for n, per_row in ((45, 1), (45, 4), (300, 1), (300, 3)):   # in pieces, and (most likely) connected
        A = S.CSR.from_rows(random_rows(rng, n, per_row, p), n, prime=p)
        whole = S.charpoly(A)
        assert S.charpoly(A, split=True).tobytes() == whole.tobytes()
        with S.DeviceCSR(A) as D:
            assert S.charpoly(D, split=True).tobytes() == whole.tobytes()


def test_block_over_the_limit_is_refused_by_name(S):
    p, n = 127, 2 + 1025
    rows = [[(0, 3)], []] + [[(2 + (i + 1) % 1025, 1)] for i in range(1025)]   # two 1 x 1 blocks, then one cycle of 1025 indices
    A = S.CSR.from_rows(rows, n, prime=p)
    buf = (C.c_int32 * (n + 4))(*([SENTINEL] * (n + 4)))
    lib = S._abi.lib()
    assert lib.spasm_amd_charpoly_split(A.data, C.cast(buf, I32P)) == -1
    assert S._abi.last_error() == "spasm_amd_charpoly_split: block 2: characteristic polynomial limited to n <= 1024 (n = 1025)"
    with S.DeviceBlocks(A, index=True) as X:
        assert X.shapes()[0].tolist() == [1, 1, 1025]
        for fn in (lib.spasm_amd_blocks_charpoly, lib.spasm_amd_blocks_charpoly_factors):
            assert fn(X._need(), C.cast(buf, I32P)) == -1
            assert "block 2: characteristic polynomial limited to n <= 1024 (n = 1025)" in S._abi.last_error()
    assert all(v == SENTINEL for v in buf)


def test_empty_matrix_and_identity(S):
    E = S.CSR.from_rows([], 0, prime=127)
    check(S.charpoly(E, split=True), [1], 127)
    with S.DeviceBlocks(E, index=True) as X:
        assert len(X) == 0 and X.index is True
        check(X.charpoly(), [1], 127)
        assert X.charpoly_factors() == []
    assert S.charpoly_split_stats()["launches"] == 0
    n = 1000
    for p in (3, P16, P32):
        I = S.CSR.from_rows([[(i, 1)] for i in range(n)], n, prime=p)
        check(S.charpoly(I, split=True), [comb(n, k) * (-1) ** (n - k) for k in range(n + 1)], p)
        st = S.charpoly_split_stats()
        assert (st["blocks"], st["lds_path"], st["global_path"], st["product_levels"]) == (n, n, 0, 10)
