"""The election of batch_eliminate (csrc/batch.hpp) beyond the first block of image rows, through every entry that runs it:
echelonize_batch / rank_batch / kernel_batch (k_batch_elim), solve_batch (k_solve_elim) and BatchSolver (k_solver_factor, then
the sparse and the dense apply).

The kernel scans the image rows in blocks of BS threads (64, 128, 256, 512 by class), one candidate per wave into a mailbox whose
two halves alternate (par flips after every block), and stops at the first block with a hit.  Random matrices put the first
non-zero of a column near the top, so the older sweeps elect inside the first block only and everything that depends on the block
(the later iterations of the base loop, base + wave * 64 + ffs, the parity after more than one flip, a pivot row in a bitset word
far from word 0, the partial last block) runs there with the result "no pivot".  The matrices here are built so that the elected
row of every column is known in advance and lies where those pieces matter; the file proves the construction on the host
(host_elected_rows) before it asks the device.

Every expected value is an exact integer elimination on the host: host_rref, host_elected_rows (test_gpu_batch.py) and
host_solve (test_gpu_solve_batch.py), int64 for p < 2^31 and Python integers above.

The constants, restated from csrc/batch.hpp and engine.hip (batch_fast, solve_shape, solve_fits), are CLASSES, LIMIT and PAD_CAP
below; batch_shape and solve_shape are the host rules for stride and class, and the launch counts of the calls (one elimination
launch per class that occurs) pin what they predict."""
import numpy as np
import pytest
from conftest import LM
from test_gpu_batch import balanced_rows, host_elected_rows, host_rref, lu_bytes, to_csr
from test_gpu_solve_batch import bal, check_system, host_solve, make_csr, raw

pytestmark = pytest.mark.gpu

CLASSES = [(1024, 64), (4096, 128), (12288, 256), (34816, 512)]  # kBatchClass: image words, threads
LIMIT, PAD_CAP = 32768, 34816                                     # BATCH_LIMIT, BATCH_PAD_CAP
BIG = (2147483647, 4294967291)


def batch_shape(n, m):
    """(class, stride) of an n x m matrix of the batch: ld = m + 1 for even m while n * (m + 1) fits the largest class, else m; the
    class is the first whose cap holds max(n * ld, n, m)"""
    ld = m + 1 if m % 2 == 0 and n * (m + 1) <= PAD_CAP else m
    key = max(n * ld, n, m)
    return next(c for c, (cap, _) in enumerate(CLASSES) if key <= cap), ld


def solve_shape(n, m, K):
    """(class, slab width, stride) of a system A (n x m) with K right-hand sides: the image has m rows and n + w columns"""
    assert m * (n + 1) <= LIMIT  # solve_fits
    for c, (cap, _) in enumerate(CLASSES):
        fit = cap // m - n
        if fit >= K or c == len(CLASSES) - 1:
            break
    w = min(K, fit)
    ld = n + w
    if ld % 2 == 0:
        if m * (ld + 1) <= CLASSES[c][0]:
            ld += 1
        elif 1 < w < K:
            w, ld = w - 1, n + w - 1
    return c, w, ld


# ---------------------------------------------------------------------------------------------------------------------------------
# the construction
# ---------------------------------------------------------------------------------------------------------------------------------
def targets(BS, m):
    """m distinct rows of an image of n = 2 * BS + 3 rows (two full blocks and a last one of three rows), one per column, in the
    order the election is to take them.  First the last row of the partial block; then, as far as m reaches, both sides of the block
    edges, the wave edge 63 | 64, the bitset word edges 31 | 32 | 33 and row 0, then further rows around block, wave and word edges.
    The order after the first is a zigzag (lowest, highest, second lowest, ...): successive elections end in different blocks, after
    a different number of parity flips."""
    n = 2 * BS + 3
    wanted = [n - 1, BS - 1, BS, BS + 1, 2 * BS - 1, 2 * BS, 0, 32, 31, 33, 63, 64,
              n - 2, BS + 32, BS + 63, BS + 64, 2 * BS - 32, 2 * BS - 33, BS + 31, 1, BS - 2, 2 * BS - 2, BS + 2, 95, 96, 65, 30,
              BS + BS // 2, BS + 33, 2 * BS - 31, 2, 127, 128, 129, BS // 2, 2 * BS - 64, 2 * BS - 65]
    rows = []
    for t in wanted:
        if 0 <= t < n and t not in rows:
            rows.append(t)
    assert len(rows) >= m
    rest = sorted(rows[1:m])
    T = [rows[0]]
    while rest:
        T.append(rest.pop(0))
        if rest:
            T.append(rest.pop())
    return T


def designed(BS, m, p, rng, drop=()):
    """(D, T, decoys): the n x m image (Python integers in [0, p)) whose election order is T.  Row T[c] is zero left of column c and
    non-zero from c on; a decoy is a non-zero multiple of row T[c] at a row BELOW it (a larger index, so the scan meets T[c] first):
    the elimination of column c must zero it, and a decoy that survives is elected at column c + 1, in another place.  Every other
    row is zero.  drop: columns whose target row and decoys are left out, so that the column finds no pivot in any block."""
    n = 2 * BS + 3
    full = targets(BS, m)
    D = np.zeros((n, m), dtype=object)
    for c, t in enumerate(full):
        D[t, c:] = [int(v) for v in rng.integers(1, p, size=m - c)]
    free = [i for i in range(n) if i not in full]
    decoys = {}
    for c in range(1, m):
        below = [i for i in free if i > full[c] and i not in decoys]
        later = [i for i in below if min(i // BS, 2) > min(full[c] // BS, 2)]
        if below:  # in a later block of rows than its target where there is one / next to its target
            d = later[int(rng.integers(0, len(later)))] if c % 2 == 1 and later else below[0]
            D[d] = (int(rng.integers(1, p)) * D[full[c]]) % p
            decoys[d] = c
    for c in drop:
        D[full[c]] = 0
        for d in [d for d, cc in decoys.items() if cc == c]:
            D[d] = 0
            del decoys[d]
    return D, [t for c, t in enumerate(full) if c not in drop], decoys


def dropped_columns(BS, m):
    """two inner columns to leave without pivot: the first whose target lies in the first block and the first whose target lies
    beyond it; columns that follow still elect, some of them beyond the first block"""
    T = targets(BS, m)
    ca = next(c for c in range(1, m - 1) if T[c] < BS)
    cb = next(c for c in range(1, m - 1) if T[c] >= BS)
    assert any(T[c] >= BS for c in range(max(ca, cb) + 1, m))
    return tuple(sorted((ca, cb)))


def guard(D, p, T, BS, decoys=None):
    """the construction, proven on the host: the election takes T in that order, a third of it or more beyond the first block, and
    every one of the three blocks of rows is hit"""
    assert host_elected_rows(D, p) == T
    assert len(set(T)) == len(T) and T != sorted(T) and T != sorted(T, reverse=True)
    assert 3 * sum(t >= BS for t in T) >= len(T)
    assert {min(t // BS, 2) for t in T} == {0, 1, 2}
    if decoys is not None:  # every decoy holds entries, all of which the elimination has to remove
        assert decoys and all(np.any(D[d] != 0) for d in decoys) and not set(decoys) & set(T)


def p_array(fact, n, m):
    return np.ctypeslib.as_array(fact.data.contents.p, (max(n, m, 1),))[:n].tolist()


def kernel_rows(R, piv, m, p):
    """the kernel vectors in the order and layout of kernel_batch: per free column f ascending, (pivot column of row k, R[k][f]) in
    k order, then (f, -1)"""
    want = balanced_rows(R, p)
    free = [f for f in range(m) if f not in piv]
    return [[(piv[k], v) for k in range(len(piv)) for (j, v) in want[k] if j == f] + [(f, -1)] for f in free]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. constructed election order through echelonize_batch, rank_batch, kernel_batch
# ---------------------------------------------------------------------------------------------------------------------------------
# BS -> m.  n = 2 * BS + 3 and m is odd, so ld = m and the image has n * m = 917, 3885, 11845, 31837 words: above the cap of the class
# below (none, 1024, 4096, 12288) and inside its own (1024, 4096, 12288, 34816).
TALL = {64: 7, 128: 15, 256: 23, 512: 31}
TINY = [(1, 1), (3, 2), (2, 3), (3, 5)]  # the last one without entries


def test_the_shapes_sit_in_their_classes():
    words = []
    for c, (BS, m) in enumerate(TALL.items()):
        n = 2 * BS + 3
        assert CLASSES[c][1] == BS and m % 2 == 1 and batch_shape(n, m) == (c, m)
        assert n * m <= CLASSES[c][0] and n * m <= LIMIT and (c == 0 or n * m > CLASSES[c - 1][0])
        words.append(n * m)
    assert words == [917, 3885, 11845, 31837]
    for (n, m) in TINY:
        assert batch_shape(n, m)[0] == 0


@pytest.mark.parametrize("p", [65521, 127, 2147483647, 4294967291])
def test_designed_election_order_in_every_class(S, O, p):
    rng = np.random.default_rng(p % 100003)
    cases = []  # (BS, D, T, dropped columns)
    for BS, m in TALL.items():
        if p in BIG and BS > 128:
            continue  # (the Python-integer references of the two large classes would take seconds)
        for drop in ((), dropped_columns(BS, m)):
            D, T, decoys = designed(BS, m, p, rng, drop)
            guard(D, p, T, BS, decoys)
            assert len(T) == m - len(drop)
            # a decoy in a later block than its target: the factor pass and the update reach past the block of the pivot
            full = targets(BS, m)
            assert any(d // BS > full[c] // BS for d, c in decoys.items())
            cases.append((BS, D, T, drop))
    for k, (n, m) in enumerate(TINY):
        D = np.zeros((n, m), dtype=object)
        if k < 3:
            D[:, :] = [[int(v) for v in row] for row in rng.integers(1, p, size=(n, m))]
        cases.insert(2 * k + 1, (0, D, None, ()))
    mats = [to_csr(S, D, p, rng) for _, D, _, _ in cases]
    ncls = len({batch_shape(*D.shape)[0] for _, D, _, _ in cases})

    facts = S.echelonize_batch(mats)
    st = S.batch_stats()
    print("batch_stats", st)
    assert st["matrices"] == st["lds_path"] == len(mats) and st["general_path"] == 0 and st["chunks"] == 1
    assert st["launches"] == ncls + 2  # one elimination per class, the scan, the pack
    assert st["max_image_words"] == max(D.shape[0] * batch_shape(*D.shape)[1] for _, D, _, _ in cases)
    ranks = S.rank_batch(mats)
    assert S.batch_stats()["launches"] == ncls and S.batch_stats()["lds_path"] == len(mats)
    Ks = S.kernel_batch(mats)
    assert S.batch_stats()["lds_path"] == len(mats)

    for idx, ((BS, D, T, drop), A, fact, rank, K) in enumerate(zip(cases, mats, facts, ranks, Ks)):
        n, m = D.shape
        where = f"matrix {idx}: {n} x {m} mod {p}, class of {BS} threads, without pivot: {drop}"
        R, piv = host_rref(D, p)
        if T is None:
            T = host_elected_rows(D, p)
        else:
            assert piv == [c for c in range(m) if c not in drop], where
            # the matrix alone: its image is the largest of the call, and nothing of the result depends on the neighbours
            alone = S.echelonize_batch([A])
            assert S.batch_stats()["max_image_words"] == n * m, where
            assert lu_bytes(alone[0]) == lu_bytes(fact), where
        assert fact.r == rank == len(piv) == len(T), where
        want_qinv = [-1] * m
        for k, c in enumerate(piv):
            want_qinv[c] = k
        assert np.asarray(fact.qinv).tolist() == want_qinv, where
        assert p_array(fact, n, m) == T + [i for i in range(n) if i not in T], where
        assert fact.U.shape == (fact.r, m) and fact.U.rows() == balanced_rows(R, p), where
        assert K.shape == (m - fact.r, m) and K.prime == p, where
        vectors = kernel_rows(R, piv, m, p)
        assert K.rows() == vectors, where
        if drop:
            assert len(vectors) == 2 and all(len(v) > 1 for v in vectors), where
            assert S.factorization_verify(A, fact, 500 + idx), where
            assert O.echelonize(A, **LM).r == fact.r, where


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. extremes of the row scan, and of the column bitset
# ---------------------------------------------------------------------------------------------------------------------------------
# (n, m) -> threads.  1024 x 1: the last shape of class 0, 16 blocks of 64 rows, the top of its 32-word bitset.  1025 x 1: the first
# shape of class 1.  32768 x 1: 64 blocks of 512 rows, 64 flips of the parity in one election.  16384 x 2: the even stride that is
# not padded (16384 * 3 = 49152 > 34816), rows at words 2 * i.
SCAN = {(1024, 1): 64, (1025, 1): 128, (32768, 1): 512, (16384, 2): 512}


def scan_rows(n, BS):
    return [n - 1, BS - 1, BS, n - 2]


@pytest.mark.parametrize("p", [65521, 4294967291])
def test_a_lone_row_at_the_extremes_of_the_scan(S, p):
    rng = np.random.default_rng(11 + p % 1000)
    cases = []
    for (n, m), BS in SCAN.items():
        c, ld = batch_shape(n, m)
        assert CLASSES[c][1] == BS and ld == m
        for d in scan_rows(n, BS):
            D = np.zeros((n, m), dtype=object)
            D[d] = [int(v) for v in rng.integers(1, p, size=m)]
            elected = [d]
            if m == 2:  # row d - 1 holds the second column alone: p = (d, d - 1), against the order of the rows
                D[d - 1, 1] = int(rng.integers(1, p))
                elected.append(d - 1)
            cases.append((D, elected))
    assert {batch_shape(*D.shape)[0] for D, _ in cases} == {0, 1, 3}
    mats = []
    for D, elected in cases:
        rows = [[] for _ in range(D.shape[0])]
        for i in elected:
            rows[i] = [(j, int(D[i, j])) for j in reversed(range(D.shape[1])) if D[i, j]]
        mats.append(S.CSR.from_rows(rows, D.shape[1], prime=p))
    facts = S.echelonize_batch(mats)
    st = S.batch_stats()
    assert st["lds_path"] == len(mats) and st["general_path"] == 0 and st["launches"] == 3 + 2 and st["max_image_words"] == 32768
    ranks = S.rank_batch(mats)
    Ks = S.kernel_batch(mats)
    for (D, elected), fact, rank, K in zip(cases, facts, ranks, Ks):
        n, m = D.shape
        where = f"{n} x {m} mod {p}, rows {elected}"
        R, piv = host_rref(D, p)
        assert host_elected_rows(D, p) == elected and piv == list(range(m)), where
        assert fact.r == rank == m and np.asarray(fact.qinv).tolist() == list(range(m)), where
        pp = p_array(fact, n, m)
        assert pp[:m] == elected, where
        assert pp[m:] == [i for i in range(n) if i not in elected], where
        assert fact.U.rows() == balanced_rows(R, p) == [[(c, 1)] for c in range(m)], where
        assert K.shape == (0, m), where


# 1 x m: the pivot COLUMN at the edges of the column bitset and of kernel mode's popcount prefix (woff).  1 x 1023 is the last shape
# of class 0 (the top of its 32 words); 1 x 1024 is padded to ld = 1025 and so, like 1 x 1025, the first of class 1; 1 x 32768 (ld =
# 32769) fills the 1024 words of class 3.
WIDE = {1023: 64, 1024: 128, 1025: 128, 32768: 512}


@pytest.mark.parametrize("p", [65521, 4294967291])
def test_a_lone_pivot_column_at_the_extremes_of_the_bitset(S, p):
    rng = np.random.default_rng(13 + p % 1000)
    cases = []
    for m, BS in WIDE.items():
        c, ld = batch_shape(1, m)
        assert CLASSES[c][1] == BS and ld == (m if m % 2 else m + 1)
        for j in (0, 31, 32, m - 33, m - 1):
            D = np.zeros((1, m), dtype=object)
            D[0, j] = int(rng.integers(1, p))
            for f in {j + 1, j + 31, j + 32, j + 33, m - 33, m - 32, m - 1} | set(range(j + 5, m, 97)):
                if j < f < m:
                    D[0, f] = int(rng.integers(1, p))
            cases.append((D, j))
    mats = []
    for D, j in cases:
        cols = [int(c) for c in np.nonzero(D[0])[0]]
        mats.append(S.CSR.from_rows([[(c, int(D[0, c])) for c in (cols[k] for k in rng.permutation(len(cols)))]], D.shape[1], prime=p))
    facts = S.echelonize_batch(mats)
    st = S.batch_stats()
    assert st["lds_path"] == len(mats) and st["general_path"] == 0 and st["launches"] == 3 + 2 and st["max_image_words"] == 32769
    assert S.rank_batch(mats) == [1] * len(mats)
    Ks = S.kernel_batch(mats)
    assert S.batch_stats()["lds_path"] == len(mats)
    for (D, j), fact, K in zip(cases, facts, Ks):
        m = D.shape[1]
        where = f"1 x {m} mod {p}, pivot column {j}"
        R, piv = host_rref(D, p)
        assert piv == [j] and R.shape == (1, m), where
        assert fact.r == 1 and np.asarray(fact.qinv).tolist() == [-1] * j + [0] + [-1] * (m - 1 - j), where
        row = balanced_rows(R, p)[0]
        assert fact.U.rows() == [row], where
        # the vectors as arrays: free column f ascending; (j, R[0][f]) first when f > j holds an entry, then (f, -1)
        r0 = dict(row)
        free = [f for f in range(m) if f != j]
        lens = np.array([2 if f in r0 else 1 for f in free], dtype=np.int64)
        wj, wx = [], []
        for f in free:
            if f in r0:
                wj.append(j)
                wx.append(r0[f])
            wj.append(f)
            wx.append(-1)
        assert K.shape == (m - 1, m) and K.prime == p, where
        nz = int(lens.sum())
        assert np.array_equal(np.asarray(K.p[: m], dtype=np.int64), np.concatenate([[0], np.cumsum(lens)])), where
        assert np.array_equal(np.asarray(K.j[:nz], dtype=np.int64), np.array(wj, dtype=np.int64)), where
        assert np.array_equal(np.asarray(K.x[:nz], dtype=np.int64), np.array(wx, dtype=np.int64)), where


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the same core through the transposed image: solve_batch, BatchSolver.solve, BatchSolver.solve_dense
# ---------------------------------------------------------------------------------------------------------------------------------
# BS -> (n, K) of A = D^T: A has n rows and m = 2 * BS + 3 columns, so the image has m rows (the columns of A) and n + K columns.
# solve_fits: m * (n + 1) = 786, 3367, 10815, 29783 <= 32768.  Class (the first with cap // m - n >= K):
#   131 x (5 + 2):   1024 // 131 = 7, 7 - 5 = 2 >= 2: class 0.  ld = 7, 131 * 7 = 917.  (n = 5 and not 4: the deficient variant
#                    loses two elections, and three are the fewest that can still end in each of the three blocks of rows.)
#   259 x (12 + 2):  1024 // 259 = 3 < 12; 4096 // 259 = 15, 15 - 12 = 3 >= 2: class 1.  n + K = 14 is even and 259 * 15 = 3885 <=
#                    4096: the padded stride, ld = 15.
#   515 x (20 + 3):  4096 // 515 = 7 < 20; 12288 // 515 = 23, 23 - 20 = 3 >= 3: class 2.  ld = 23, 515 * 23 = 11845.
#   1027 x (28 + 3): 12288 // 1027 = 11 < 28; 34816 // 1027 = 33, 33 - 28 = 5 >= 3: class 3.  ld = 31, 1027 * 31 = 31837.
# The factor step of BatchSolver runs the image with the m identity columns in slabs (solve_shape with K = m), which no class
# below the last holds for these m: all four factor in class 3 (512 threads), where the rows of the two small systems are one
# block and those of the two large ones (515 = 512 + 3, 1027 = 2 * 512 + 3) two and three.  The applies read what the factor
# elected.
SYSTEMS = {64: (5, 2), 128: (12, 2), 256: (20, 3), 512: (28, 3)}


def test_the_systems_sit_in_their_classes():
    want = {64: (0, 2, 7, 917), 128: (1, 2, 15, 3885), 256: (2, 3, 23, 11845), 512: (3, 3, 31, 31837)}
    for c, (BS, (n, K)) in enumerate(SYSTEMS.items()):
        m = 2 * BS + 3
        cls, w, ld = solve_shape(n, m, K)
        assert CLASSES[c][1] == BS and (cls, w, ld, m * ld) == want[BS]
        assert m * ld <= CLASSES[c][0] and (c == 0 or m * ld > CLASSES[c - 1][0])
        assert solve_shape(n, m, m)[0] == 3  # the factor step


DEPENDENT = (2, 3)  # row 2 of A becomes a copy of row 0 and row 3 a combination of rows 0 and 1; the rows after them still elect


def build_system(BS, p, rng, deficient):
    """(A, B, elected image rows): A = D^T for a designed image D.  deficient: the image columns (rows of A) r1, r2 lose their target
    rows and become a copy of column 0 and a combination of columns 0 and 1: candidates that find no pivot in any block."""
    n, K = SYSTEMS[BS]
    m = 2 * BS + 3
    drop = DEPENDENT if deficient else ()
    D, T, _ = designed(BS, n, p, rng, drop)
    if deficient:
        r1, r2 = drop
        D[:, r1] = D[:, 0]
        D[:, r2] = (int(rng.integers(1, p)) * D[:, 0] + int(rng.integers(1, p)) * D[:, 1]) % p
    guard(D, p, T, BS)
    A = D.T.copy()
    outside = [i for i in range(m) if i not in T]
    B = np.zeros((K, m), dtype=object)
    for k in range(K):
        y = np.array([int(v) for v in rng.integers(0, p, size=n)], dtype=object)
        B[k] = (y @ A) % p  # (Python integers: a sum of n products below p^2 passes 2^63 for the primes near 2^31)
        if k % 2 == 1:  # a unit entry on a column of A that is no elected image row: the last such column, then any
            j = outside[-1] if k == 1 else outside[int(rng.integers(0, len(outside)))]
            B[k, j] = (B[k, j] + 1) % p
    dt = object if p >= 2 ** 31 else np.int64
    return A.astype(dt), B.astype(dt), T


@pytest.mark.parametrize("deficient", [False, True], ids=["full", "deficient"])
@pytest.mark.parametrize("p", [65521, 127, 2147483647, 4294967291])
def test_solves_elect_beyond_the_first_block(S, p, deficient):
    rng = np.random.default_rng(p % 100003 + (7 if deficient else 0))
    sizes = [BS for BS in SYSTEMS if not (p in BIG and BS > 128)]
    systems = [build_system(BS, p, rng, deficient) for BS in sizes]
    refs = []
    for BS, (A, B, T) in zip(sizes, systems):
        n, K = SYSTEMS[BS]
        Xw, okw, basis = host_solve(A, B, p)
        gone = DEPENDENT if deficient else ()
        assert basis == [c for c in range(n) if c not in gone] and len(basis) == len(T)
        assert okw.tolist() == [k % 2 == 0 for k in range(K)] and okw.any() and not okw.all()
        refs.append((Xw, okw, basis))
    As = [make_csr(S, A, p, rng) for A, _, _ in systems]
    Bs = [make_csr(S, B, p, rng) for _, B, _ in systems]

    X, ok = S.solve_batch(As, Bs)
    st = S.solve_stats()
    print("solve_stats", st)
    assert st["systems"] == st["lds_path"] == st["jobs"] == len(systems) and st["general_path"] == 0
    unsolved = 0
    for BS, (A, B, T), x, o, (Xw, okw, basis) in zip(sizes, systems, X, ok, refs):
        unsolved += check_system(x, o, A, B, p)  # ok exactly, X entry for entry against host_solve
        nz = int(x.p[x.n])
        assert set(x.j[:nz].tolist()) <= set(basis), BS
    assert st["unsolved"] == unsolved == sum(SYSTEMS[BS][1] // 2 for BS in sizes)
    assert st["launches"] == len(systems) + 2  # one elimination per class, the scan, the pack

    with S.BatchSolver(As) as sv:
        info = sv.info()
        assert info["systems"] == info["lds_path"] == len(systems) and info["general_path"] == 0
        assert sv.ranks == [len(T) for _, _, T in systems]
        for i, (_, _, basis) in enumerate(refs):
            assert sv.basis(i).tolist() == basis
        X2, ok2 = sv.solve(Bs)
        st2 = S.solver_stats()
        assert st2["lds_path"] == len(systems) and st2["general_path"] == 0 and st2["unsolved"] == unsolved
        assert [raw(x) for x in X2] == [raw(x) for x in X]
        assert [o.tolist() for o in ok2] == [o.tolist() for o in ok]
        # the dense apply: system i owns its m rows of B and its n rows of X; the columns past its K are zero right-hand sides
        kmax = max(SYSTEMS[BS][1] for BS in sizes)
        Bd = np.zeros((sum(A.shape[1] for A, _, _ in systems), kmax), dtype=np.int32)
        Xwant = np.zeros((sum(A.shape[0] for A, _, _ in systems), kmax), dtype=np.int32)
        okwant = np.ones((len(systems), kmax), dtype=bool)
        r0 = c0 = 0
        for i, ((A, B, _), (Xw, okw, _)) in enumerate(zip(systems, refs)):
            n, m = A.shape
            K = B.shape[0]
            Bd[c0:c0 + m, :K] = np.array([[bal(v, p) for v in row] for row in B.T], dtype=np.int64)
            Xwant[r0:r0 + n, :K] = np.array([[bal(v, p) for v in row] for row in Xw.T], dtype=np.int64)
            okwant[i, :K] = okw
            r0, c0 = r0 + n, c0 + m
        Xd, okd = sv.solve_dense(Bd)
        assert sv.dense_info()["general_path"] == 0
        assert np.array_equal(okd, okwant)
        assert np.array_equal(Xd, Xwant)
        # and against the CSR rows of the sparse entries
        r0 = 0
        for (A, B, _), x in zip(systems, X):
            for k, row in enumerate(x.rows()):
                col = np.zeros(A.shape[0], dtype=np.int32)
                for c, v in row:
                    col[c] = v
                assert np.array_equal(Xd[r0:r0 + A.shape[0], k], col)
            r0 += A.shape[0]
