"""The block split on the device (S.DeviceBlocks, csrc/blocks.hpp) against the host split Block.from_csr, which is the yardstick and
not the code under test: same maps, same blocks entry for entry, and the same results from the three consumers that read the blocks
where they lie."""
import numpy as np
import pytest
from conftest import LM
from test_blocks import make_block_matrix

pytestmark = pytest.mark.gpu

P0 = 42013


def from_cols(S, rows, m, prime=P0, seed=1, values=None):
    """CSR whose row i holds the columns rows[i] in that order, with non-zero balanced values"""
    rng = np.random.default_rng(seed)
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    j = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if len(rows) and p[-1] else np.zeros(0, dtype=np.int64)
    x = S.balanced(rng.integers(1, prime, size=len(j)), prime) if values is None else np.asarray(values, dtype=np.int32)
    return S.CSR.from_arrays(len(rows), m, p, j, x, prime=prime)


def shuffled(rows, m, seed):
    """rows and columns permuted, the entries of a row in a random order too"""
    rng = np.random.default_rng(seed)
    rperm, cperm = rng.permutation(len(rows)), rng.permutation(m)
    out = [None] * len(rows)
    for i, r in enumerate(rows):
        out[rperm[i]] = rng.permutation(cperm[np.asarray(r, dtype=np.int64)]) if len(r) else []
    return out


def path_matrix(S):
    n = 5000
    return from_cols(S, shuffled([[i, i + 1] for i in range(n)], n + 1, 5), n + 1)


def star_matrix(S):
    n = 4096
    return from_cols(S, shuffled([[0, 1 + i] for i in range(n)], n + 1, 6), n + 1)


def long_row_matrix(S):
    rng = np.random.default_rng(7)
    L, m = 70000, 70000 + 300
    rows = [list(range(L))]
    for k in range(200):  # short rows: some hang on the long row, the others make components of their own
        own = [L + k, L + (k + 1 if k % 3 else k)]
        rows.append(sorted(set(own + ([int(rng.integers(0, L))] if k % 4 == 0 else []))))
    return from_cols(S, shuffled(rows, m, 8), m)


def wave_boundary_matrix(S):
    rows, c = [], 1
    for ln in (63, 64, 65):
        rows.append([0] + list(range(c, c + ln - 1)))
        c += ln - 1
    return from_cols(S, shuffled(rows, c + 2, 9), c + 2)


def many_small_matrix(S):
    rows, c = [], 0
    for k in range(3000):
        if k % 2 == 0:
            rows.append([c])
            c += 1
        else:
            rows += [[c, c + 1], [c, c + 1]]
            c += 2
    return from_cols(S, shuffled(rows, c, 10), c, seed=2)


def big_and_small_matrix(S):
    rng = np.random.default_rng(11)
    rows, c = [], 0
    for (a, b) in [(200, 200)] + [(5, 6)] * 50:
        D = rng.random((a, b)) < (0.3 if a == 200 else 0.6)
        D[:, 0] = True  # connected
        D[0, :] = True
        rows += [list(c + np.nonzero(D[i])[0]) for i in range(a)]
        c += b
    rows[3] = list(rows[1])  # a rank deficiency in the large block
    return from_cols(S, shuffled(rows, c, 12), c, seed=3)


def no_entries_matrix(S):
    return from_cols(S, [[] for _ in range(7)], 5)


def linked_by_zero_matrix(S):
    """row 0 holds column 0 twice; the explicit zero at (1, 1) is the only link between {row 0, columns 0, 1} and {row 1, column 2};
    row 2 with column 3 stays apart"""
    return from_cols(S, [[0, 0, 1], [1, 2], [3]], 4, values=[5, 6, 7, 0, 9, 4])


BUILDERS = {
    "fixture": lambda S: make_block_matrix(S)[0],
    "fixture_p127": lambda S: make_block_matrix(S, seed=4, p=127)[0],
    "fixture_p65521": lambda S: make_block_matrix(S, seed=5, p=65521)[0],
    "fixture_pmax": lambda S: make_block_matrix(S, seed=6, p=0xFFFFFFFB)[0],
    "path": path_matrix,
    "star": star_matrix,
    "long_row": long_row_matrix,
    "wave_boundary": wave_boundary_matrix,
    "many_small": many_small_matrix,
    "big_and_small": big_and_small_matrix,
    "no_entries": no_entries_matrix,
    "zero_rows": lambda S: from_cols(S, [], 5),
    "zero_cols": lambda S: from_cols(S, [[] for _ in range(6)], 0),
    "linked_by_zero": linked_by_zero_matrix,
}
CONSUMED = ["fixture", "many_small", "big_and_small"]

_cache = {}


def case(S, name):
    """(A, Block.from_csr(A)): built once, shared, never changed"""
    if name not in _cache:
        A = BUILDERS[name](S)
        _cache[name] = (A, S.Block.from_csr(A))
    return _cache[name]


def same_matrix(X, Y):
    nz = int(X.p[X.n])
    return X.shape == Y.shape and X.prime == Y.prime and np.array_equal(X.p, Y.p) and np.array_equal(X.j[:nz], Y.j[:nz]) and np.array_equal(X.x[:nz], Y.x[:nz])


def same_split(D, H):
    assert len(D) == len(H)
    assert D.row2block == H.row2block and D.col2block == H.col2block
    assert D.block2row == H.block2row and D.block2col == H.block2col
    for b, (X, Y) in enumerate(zip(D.blocks, H.blocks)):
        assert same_matrix(X, Y), b


@pytest.mark.parametrize("name", list(BUILDERS))
def test_device_split_equals_host_split(S, name):
    A, H = case(S, name)
    with S.DeviceBlocks(A) as DB:
        assert len(DB) == len(H) and DB.shape == A.shape
        info = DB.info()
        rows, cols, nz = DB.shapes()
        D = DB.to_block()
    same_split(D, H)
    assert D.to_csr().rows() == A.rows()
    assert info["blocks"] == len(H) and (info["n"], info["m"], info["nnz"]) == (A.n, A.m, S.nnz(A))
    assert rows.tolist() == [X.n for X in H.blocks] and cols.tolist() == [X.m for X in H.blocks]
    assert nz.tolist() == [S.nnz(X) for X in H.blocks]
    assert info["blocks_without_entries"] == sum(1 for X in H.blocks if S.nnz(X) == 0)
    assert info["largest_nnz"] == max([S.nnz(X) for X in H.blocks], default=0)


def test_expected_shapes_of_the_special_cases(S):
    """the host split itself gives what the cases were built for"""
    assert len(case(S, "path")[1]) == 1 and len(case(S, "star")[1]) == 1
    assert len(case(S, "no_entries")[1]) == 12 and len(case(S, "zero_rows")[1]) == 5 and len(case(S, "zero_cols")[1]) == 6
    assert len(case(S, "many_small")[1]) == 3000
    assert len(case(S, "big_and_small")[1]) == 51
    assert len(case(S, "linked_by_zero")[1]) == 2
    assert max(X.n * X.m for X in case(S, "big_and_small")[1].blocks) > 32768


def test_from_csr_device_keyword(S):
    A, H = case(S, "fixture")
    same_split(S.Block.from_csr(A, device=True), H)


@pytest.mark.parametrize("name", ["fixture", "many_small"])
def test_resident_input_gives_the_same_split(S, name):
    A, H = case(S, name)
    with S.DeviceCSR(A) as R, S.DeviceBlocks(R) as DB, S.DeviceBlocks(A) as DA:
        mr, ma = DB.maps(), DA.maps()
        assert all(np.array_equal(mr[k], ma[k]) for k in ma)
        for b in range(len(DA)):
            assert same_matrix(DB.fetch(b), DA.fetch(b)), b
        same_split(DB.to_block(), H)


@pytest.mark.parametrize("name", ["path", "star"])
def test_two_handles_are_byte_identical(S, name):
    A, _ = case(S, name)
    with S.DeviceBlocks(A) as D1, S.DeviceBlocks(A) as D2:
        m1, m2 = D1.maps(), D2.maps()
        assert all(m1[k].tobytes() == m2[k].tobytes() for k in m1)
        assert len(D1) == len(D2)
        for b in range(len(D1)):
            X, Y = D1.fetch(b), D2.fetch(b)
            nz = int(X.p[X.n])
            assert X.p.tobytes() == Y.p.tobytes() and X.j[:nz].tobytes() == Y.j[:nz].tobytes() and X.x[:nz].tobytes() == Y.x[:nz].tobytes()


@pytest.mark.parametrize("name", CONSUMED)
def test_rank_from_the_device_blocks(S, name):
    A, H = case(S, name)
    want = S.blocks.rank(H, batched=True)
    host_stats = S.batch_stats()
    with S.DeviceBlocks(A) as DB:
        got = S.blocks.rank(DB)
        dev_stats = S.batch_stats()
        per_block = DB.rank()
    assert got == want == S.rank(A)
    assert per_block == S.rank_batch(H.blocks)
    for k in ("matrices", "lds_path", "general_path"):
        assert dev_stats[k] == host_stats[k], (k, dev_stats, host_stats)


@pytest.mark.parametrize("name", CONSUMED)
def test_echelonize_from_the_device_blocks(S, name):
    A, H = case(S, name)
    want = S.echelonize_batch(H.blocks, **LM)
    host_stats = S.batch_stats()
    with S.DeviceBlocks(A) as DB:
        E = S.blocks.echelonize(DB, **LM)
        dev_stats = S.batch_stats()
    assert (E.row2block, E.col2block, E.block2row, E.block2col) == (H.row2block, H.col2block, H.block2row, H.block2col)
    assert len(E.blocks) == len(want)
    for b, (X, Y) in enumerate(zip(E.blocks, want)):
        assert X.r == Y.r, b
        assert X.qinv.tobytes() == Y.qinv.tobytes() and X.p.tobytes() == Y.p.tobytes(), b
        assert same_matrix(X.U, Y.U), b
    for k in ("matrices", "lds_path", "general_path"):
        assert dev_stats[k] == host_stats[k], (k, dev_stats, host_stats)


@pytest.mark.parametrize("name", CONSUMED)
def test_kernel_from_the_device_blocks(S, O, name):
    A, H = case(S, name)
    with S.DeviceBlocks(A) as DB:
        K = S.blocks.kernel(DB, **LM).to_csr()
        dev_stats = S.batch_stats()
    want = O.kernel(O.echelonize(A, **LM)).rows()
    assert K.shape == (len(want), A.m)
    assert sorted(K.rows()) == sorted(want)
    S.kernel_batch(H.blocks, **LM)
    host_stats = S.batch_stats()
    for k in ("matrices", "lds_path", "general_path"):
        assert dev_stats[k] == host_stats[k], (k, dev_stats, host_stats)


@pytest.mark.parametrize("name", CONSUMED)
def test_with_L_every_block_takes_the_general_path(S, name):
    """(many_small: 3 000 blocks x 13 ms of the general path each, 39 s on an MI355X; the other two cases 0.05 s and 1.1 s)"""
    A, H = case(S, name)
    with S.DeviceBlocks(A) as DB:
        E = S.blocks.echelonize(DB, L=True, **LM)
        st = S.batch_stats()
    assert st["lds_path"] == 0 and st["general_path"] == len(H) == st["matrices"]
    for b, (X, lu) in enumerate(zip(H.blocks, E.blocks)):
        assert S.factorization_verify(X, lu, 1 + b), b


def test_owner_is_refused_with_a_handle(S):
    A, _ = case(S, "fixture")
    with S.DeviceBlocks(A) as DB:
        with pytest.raises(ValueError):
            S.blocks.rank(DB, owner=(0, 2))
    with pytest.raises(S.SpasmError, match="closed"):
        DB.rank()


def test_refusals_on_the_device(S):
    A = from_cols(S, [[0, 1], [1], [2]], 3)
    A.j[2] = 3  # == m
    with pytest.raises(S.SpasmError, match="column index"):
        S.DeviceBlocks(A)
    A.j[2] = -1
    with pytest.raises(S.SpasmError, match="column index"):
        S.DeviceBlocks(A)
    B = from_cols(S, [[0, 1], [1], [2]], 3)
    B.p[1], B.p[2] = 3, 2
    with pytest.raises(S.SpasmError, match="row pointers must not decrease"):
        S.DeviceBlocks(B)
    B.p[1], B.p[2] = 2, 3
    with S.DeviceBlocks(B) as DB:  # and the error text is cleared by the next success
        assert len(DB) == 2 and S._abi.last_error() == ""
