"""The triangular solver (csrc/trsolve.hpp, trsolve_create in engine.hip) at its fold and panel boundaries.

A. Equal-sign chains.  For p < 2^16 a lane of k_trs_push / k_trs_residual sums lazy products in i32 and the fold every TRS_FOLD
   terms is the only guard against wrapping (an i32 holds 65043 terms of halfp + 256 at p = 65521, csrc/zp.hpp).  Random residues
   never get near that; here one lane takes 70 000 terms that are all +halfp (or all -halfp).  A sum that wraps mod 2^32 is not
   a multiple of p off, so the solution and the residual come out wrong.
B. Layered matrices whose level widths sit on TRS_WIDE = 256, TRS_CHUNK = 64 and the 32-entries-per-descriptor team thresholds;
   the plan reported by TriangularSolver.stats() is compared with a restatement of the packing rule.
C. The constructions themselves, on the CPU: an independent Kahn pass finds the requested widths, and an entry-by-entry sparse
   product agrees with the right-hand sides that the GPU tests use.
D. The diagonal of a row that repeats its pivot entry millions of times with unreduced values: the sum of the raw values leaves the
   domain of zp_reduce, so trsolve_create reduces entry by entry.

Every comparison is exact integer equality against Python ints or int64 numpy."""
from types import SimpleNamespace

import numpy as np
import pytest
from test_gpu_trsolve import bal, dense_of, seq_forward, xT

gpu = pytest.mark.gpu

TRS_WIDE, TRS_CHUNK = 256, 64  # csrc/trsolve.hpp
KINDS = ["forward", "back"]


# ---- shared construction helpers --------------------------------------------------------------------------------------------------

def csr_arrays(n, m, r, c, v, p):
    """Entries (r, c, v) in the order given, gathered by row (stably): the fields of a CSR that dense_of and seq_forward read."""
    r = np.asarray(r, dtype=np.int64)
    o = np.argsort(r, kind="stable")
    ptr = np.zeros(n + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(np.bincount(r, minlength=n))
    return SimpleNamespace(n=n, m=m, p=ptr, j=np.asarray(c)[o].astype(np.int32), x=bal(np.asarray(v)[o], p), prime=p)


def on_device(S, T):
    return S.CSR.from_arrays(T.n, T.m, T.p, T.j, T.x, prime=T.prime)


def pivots(n, m, prow, pcol, kind):
    """(piv as the solver takes it, rowcol): forward q[row] = column, back p[column] = row"""
    rowcol = -np.ones(n, dtype=np.int64)
    rowcol[prow] = pcol
    if kind == "forward":
        return rowcol.astype(np.int32), rowcol
    pv = -np.ones(m, dtype=np.int32)
    pv[pcol] = prow
    return pv, rowcol


def sparse_xT(T, X):
    """x T mod p entry by entry in int64, without the dense image: |value|, |x| <= p/2 < 2^31, so a product is below 2^62, and a
    column sums fewer than 2^31 reduced terms."""
    p = T.prime
    nnz = int(T.p[T.n])
    rows = np.repeat(np.arange(T.n), np.diff(T.p))
    o = np.argsort(T.j[:nnz], kind="stable")
    cols, starts = np.unique(T.j[:nnz][o], return_index=True)
    vals, rows = T.x[:nnz].astype(np.int64)[o], rows[o]
    Xb = bal(X, p).astype(np.int64)
    out = np.zeros((T.m, Xb.shape[1]), dtype=np.int64)
    for v0 in range(0, Xb.shape[1], 8):
        prod = (vals[:, None] * Xb[rows, v0:v0 + 8]) % p
        out[cols, v0:v0 + 8] = np.add.reduceat(prod, starts, axis=0) % p
    return out


def kahn_widths(T, rowcol):
    """Level widths of the pivot graph (edge i -> k: row i has an entry on the pivot column of row k != i), frontier by frontier"""
    n, nnz = T.n, int(T.p[T.n])
    part = rowcol >= 0
    colrow = -np.ones(T.m, dtype=np.int64)
    colrow[rowcol[part]] = np.flatnonzero(part)
    rows = np.repeat(np.arange(n), np.diff(T.p))
    tgt = colrow[T.j[:nnz]]
    e = part[rows] & (tgt >= 0) & (tgt != rows)
    src, dst = rows[e], tgt[e]
    indeg = np.bincount(dst, minlength=n)
    front = np.flatnonzero(part & (indeg == 0))
    widths = []
    while front.size:
        widths.append(int(front.size))
        infront = np.zeros(n, dtype=bool)
        infront[front] = True
        hit = dst[infront[src]]
        indeg -= np.bincount(hit, minlength=n)
        hit = np.unique(hit)
        front = hit[indeg[hit] == 0]
    assert sum(widths) == int(part.sum()), "the pivot graph has a cycle"
    return widths


def pack(widths):
    """(wide panels, chunks) for a list of level widths, the rule at the top of csrc/trsolve.hpp: a level of at least TRS_WIDE
    rows is a panel of its own and closes the open chunk; narrower levels fill chunks of TRS_CHUNK positions, a level going on
    in the next chunk when one is full."""
    wide = chunks = cur = 0
    for w in widths:
        if w >= TRS_WIDE:
            wide, chunks, cur = wide + 1, chunks + (cur > 0), 0
            continue
        while w > 0:
            take = min(w, TRS_CHUNK - cur)
            cur, w = cur + take, w - take
            if cur == TRS_CHUNK:
                chunks, cur = chunks + 1, 0
    return wide, chunks + (cur > 0)


def rand_int32(rng, shape):
    return rng.integers(-(2**31), 2**31, size=shape, dtype=np.int64).astype(np.int32)


# ---- A. equal-sign chains through the fold ------------------------------------------------------------------------------------------

PRIMES_A = [65521, 32749, 65537, 0xFFFFFFFB]  # must fold; i32 without a fold would do (capacity 129 133); i64; i64
CHAINS = [(70_000, 64), (140_000, 20)]        # KW = 64, E = 1; KW = 32, kc = 20, E = 2: 70 000 > 65 043 terms in a lane either way
SMALL_CHAIN = (255, 20)                       # below TRS_WIDE: level 0 in four chunks, four pushes into one accumulator


def chain(N, k, p, kind):
    """n = N + 2, m = N + 4.  Row i < N: diagonal on column i, then (N, +h), (N+1, -h), (N+2, +h), (N+3, -h), h = p // 2; rows N
    and N + 1: the diagonal only; columns N + 2 and N + 3 without a pivot.  The diagonal is 1 (forward), or -1 on the first N rows
    and 2 on the last two (back).  Level 0 is the first N rows, level 1 the other two, fed by two descriptors of N entries; the
    residual has two columns of N entries.

    Right-hand sides, one column per case, described by the solution on the first N rows: v = 0 all +1, v = 1 all -1 (every lazy
    term is +-h exactly, of one sign), v = 2 all +h, v = 3 alternating +-1 (cannot wrap), then random residues (even v) and b
    given as unreduced int32 (odd v).  With Sx = sum of that solution, d the diagonal of the last two rows:
        x_N = (b_N - h Sx) / d,  x_{N+1} = (b_{N+1} + h Sx) / d,  residual b_{N+2} - h Sx on column N + 2, b_{N+3} + h Sx on N + 3;
    b on the two free columns makes the residual zero for even v and non-zero for odd v.
    Returns T, piv, rowcol, B, and the expected X, residual B and ok."""
    assert k >= 6
    rng = np.random.default_rng(N + k + p % 1009 + (kind == "back"))
    h = p // 2
    n, m = N + 2, N + 4
    dl, dt = (1, 1) if kind == "forward" else (-1, 2)
    i = np.arange(N)
    r = np.concatenate([np.repeat(i, 5), [N, N + 1]])
    c = np.concatenate([np.stack([i, i * 0 + N, i * 0 + N + 1, i * 0 + N + 2, i * 0 + N + 3], axis=1).ravel(), [N, N + 1]])
    v = np.concatenate([np.tile(np.array([dl, h, -h, h, -h], dtype=np.int64), N), [dt, dt]])
    T = csr_arrays(n, m, r, c, v, p)
    piv, rowcol = pivots(n, m, np.arange(n), np.arange(n), kind)

    B = np.zeros((m, k), dtype=np.int32)
    X0 = np.empty((N, k), dtype=np.int64)
    X0[:, 0], X0[:, 1], X0[:, 2], X0[:, 3] = 1, -1, h, 1 - 2 * (i & 1)
    for col in range(4, k):
        if col % 2 == 0:
            X0[:, col] = bal(rng.integers(0, p, size=N), p)
        else:  # dl = +-1 is its own inverse
            B[:N, col] = rand_int32(rng, N)
            X0[:, col] = bal(dl * B[:N, col].astype(np.int64), p)
    even = np.arange(k) % 2 == 0
    B[:N, :4] = bal(dl * X0[:, :4], p)
    B[:N, 4::2] = bal(dl * X0[:, 4::2], p)
    B[N:N + 2] = rand_int32(rng, (2, k))
    wantX = np.zeros((n, k), dtype=np.int32)
    wantX[:N] = X0
    wantB = np.zeros((m, k), dtype=np.int32)
    dinv = pow(dt, -1, p)
    for col in range(k):  # Python ints: h * Sx reaches 2^79 at p = 0xFFFFFFFB
        hs = h * int(X0[:, col].sum())
        wantX[N, col] = bal((int(B[N, col]) - hs) * dinv % p, p)
        wantX[N + 1, col] = bal((int(B[N + 1, col]) + hs) * dinv % p, p)
        d2 = 0 if even[col] else int(rng.integers(1, p))
        d3 = int(rng.integers(1, p)) if col % 4 == 3 else 0
        B[N + 2, col], B[N + 3, col] = bal((hs + d2) % p, p), bal((-hs + d3) % p, p)
        wantB[N + 2, col], wantB[N + 3, col] = bal(d2, p), bal(d3, p)
    return T, piv, rowcol, B, wantX, wantB, even


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p", PRIMES_A)
@pytest.mark.parametrize("N,k", CHAINS + [SMALL_CHAIN])
def test_chain_construction(N, k, p, kind):
    T, piv, rowcol, B, wantX, wantB, wantok = chain(N, k, p, kind)
    assert kahn_widths(T, rowcol) == [N, 2]
    # the closed forms against the entry-by-entry product: x T + residual = b
    assert np.array_equal((sparse_xT(T, wantX) + wantB) % p, B.astype(np.int64) % p)
    assert not wantB[:N + 2].any() and np.array_equal(wantok, ~wantB.any(axis=0))
    h = p // 2
    assert (wantX[:N, 0] == 1).all() and (wantX[:N, 1] == -1).all() and (wantX[:N, 2] == h).all() and wantX[:N, 3].sum() == N % 2
    if (N, k) != SMALL_CHAIN:
        E = {64: 1, 20: 2}[k]  # lanes of a 64-lane team per vector: 64 / KW
        assert N // E > (2**31 - 1) // (65521 // 2 + 256) and (N // E) * (65521 // 2) > 2**31 > (N // E) * (32749 // 2)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p", PRIMES_A)
@pytest.mark.parametrize("N,k", CHAINS)
def test_equal_sign_chain_through_the_fold(S, N, k, p, kind):
    T, piv, rowcol, B, wantX, wantB, wantok = chain(N, k, p, kind)
    with S.TriangularSolver(on_device(S, T), piv, kind) as ts:
        st = ts.stats()
        assert (st["rows"], st["levels"], st["wide_panels"], st["chunks"]) == (N + 2, 2, 1, 1)
        X, ok = ts.solve(B)
    bad = np.flatnonzero((X != wantX).any(axis=0) | (B != wantB).any(axis=0) | (ok != wantok))
    assert bad.size == 0, f"wrong vectors {bad.tolist()}: x_N {X[N, bad].tolist()} for {wantX[N, bad].tolist()}"
    assert np.array_equal(X, wantX) and np.array_equal(B, wantB) and np.array_equal(ok, wantok)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p", PRIMES_A)
def test_equal_sign_chain_below_the_wide_threshold(S, p, kind):
    """The same entries through k_trs_chunk_solve: level 0 (255 rows) is four chunks, the fourth closes on the first row of level 1
    (which it reaches through its diagonal block), the second row of level 1 is a fifth chunk fed by four pushes."""
    N, k = SMALL_CHAIN
    T, piv, rowcol, B, wantX, wantB, wantok = chain(N, k, p, kind)
    B0 = B.copy()
    with S.TriangularSolver(on_device(S, T), piv, kind) as ts:
        st = ts.stats()
        assert (st["levels"], st["wide_panels"], st["chunks"]) == (2, 0, 5) and pack([N, 2]) == (0, 5)
        X, ok = ts.solve(B)
    assert np.array_equal(X, wantX) and np.array_equal(B, wantB) and np.array_equal(ok, wantok)
    if kind == "forward":  # rows are stored in a topological order: the reference's sequential loop applies
        for col in (0, 1, 5):
            sx, sb, sok = seq_forward(T, B0[:, col], piv)
            assert np.array_equal(X[:, col], sx) and np.array_equal(B[:, col], sb) and ok[col] == sok


# ---- B. layered matrices at the panel boundaries ------------------------------------------------------------------------------------

PRIMES_B = [3, 65521, 65537, 0xFFFFFFFB]
NIDLE = 3  # rows that take no part


def layered(widths, p, rng, kind, extra_free, fan=2, feed=0.0, free_density=0.3, dup=False):
    """Level l has widths[l] participating rows, on shuffled row numbers and shuffled pivot columns.  Every row of level l + 1 has
    an entry from one row of level l; beyond that each row feeds `fan` random rows of any later level and, with probability
    `feed`, each row of the next level.  Edges go from a level to a later one only, so the levels are exactly the widths.
    extra_free columns carry no pivot (each row has an entry there with probability free_density) and NIDLE rows take no part.
    dup: every mandatory entry and a third of the entries on free columns are stored twice (two values), and a third of the
    diagonals are split into two entries whose sum is the diagonal.  Entries of a row are stored in shuffled order.
    Returns T, piv, rowcol, prow, pcol and the entry counts that decide the team shapes."""
    widths = np.asarray(widths, dtype=np.int64)
    npart, L = int(widths.sum()), len(widths)
    n, m = npart + NIDLE, npart + extra_free
    rowperm, colperm = rng.permutation(n), rng.permutation(m)
    prow, idle = rowperm[:npart], rowperm[npart:]
    pcol, free = colperm[:npart], colperm[npart:]
    ends = np.cumsum(widths)
    begs = ends - widths
    feeds_s = [rng.integers(begs[l - 1], ends[l - 1], size=widths[l]) for l in range(1, L)]
    feeds_t = [np.arange(begs[l], ends[l]) for l in range(1, L)]
    src, dst = list(feeds_s), list(feeds_t)
    for l in range(L - 1):
        s = np.repeat(np.arange(begs[l], ends[l]), fan)
        src.append(s)
        dst.append(rng.integers(ends[l], npart, size=s.size))
        if feed > 0:
            a, b = np.nonzero(rng.random((widths[l], widths[l + 1])) < feed)
            src.append(begs[l] + a)
            dst.append(ends[l] + b)
    pairs = np.unique(np.concatenate(src + [np.zeros(0, np.int64)]) * npart + np.concatenate(dst + [np.zeros(0, np.int64)]))
    src, dst = pairs // npart, pairs % npart
    fs, ff = np.nonzero(rng.random((npart, extra_free)) < free_density)
    diag = np.ones(npart, dtype=np.int64) if kind == "forward" else rng.integers(1, p, size=npart)
    ir, ic = np.nonzero(rng.random((NIDLE, m)) < 0.2)
    r = [prow[src], prow[fs], prow, idle[ir]]
    c = [pcol[dst], free[ff], pcol, ic]
    v = [rng.integers(1, p, size=src.size), rng.integers(1, p, size=fs.size), diag, rng.integers(1, p, size=ir.size)]
    if dup:
        ms, mt = np.concatenate(feeds_s), np.concatenate(feeds_t)
        pick = np.arange(fs.size) % 3 == 0
        d1 = rng.integers(1, p, size=npart)
        split = (np.arange(npart) % 3 == 0) & ((d1 - diag) % p != 0)
        v[2] = np.where(split, d1, diag)
        r += [prow[ms], prow[fs[pick]], prow[split]]
        c += [pcol[mt], free[ff[pick]], pcol[split]]
        v += [rng.integers(1, p, size=ms.size), rng.integers(1, p, size=int(pick.sum())), (diag - d1)[split] % p]
    r, c, v = np.concatenate(r), np.concatenate(c), np.concatenate(v)
    o = rng.permutation(r.size)
    T = csr_arrays(n, m, r[o], c[o], v[o], p)
    piv, rowcol = pivots(n, m, prow, pcol, kind)
    counts = SimpleNamespace(edges=int(src.size), targets=int(np.unique(dst).size), nres=int(fs.size), m=m)
    return T, piv, rowcol, prow, pcol, counts


# name -> widths and the generator's options.  The plan (wide panels, chunks) each list asks for is in test_packing_rule.
LAYERS = {
    "255": dict(widths=[255]),
    "256": dict(widths=[256]),
    "257": dict(widths=[257]),
    "63": dict(widths=[63]),
    "64": dict(widths=[64]),
    "65": dict(widths=[65]),
    "63+2": dict(widths=[63, 2]),                 # level 1 split 1 + 1
    "100+28+5": dict(widths=[100, 28, 5]),        # level 0 straddles; level 1 closes the second chunk exactly at 64
    "65x1": dict(widths=[1] * 65),                # 64 steps in one chunk, the 65th in the next
    "256+255+256": dict(widths=[256, 255, 256]),
    "300+10+300+64+64+1": dict(widths=[300, 10, 300, 64, 64, 1]),
    "40+300+40": dict(widths=[40, 300, 40]),
    # [300, 300] is two wide panels; panel 0 has one descriptor per row of level 1 (each has its mandatory entry), so
    # long_team = edges > 32 * 300 = 9600, and res_long = entries on free columns > 32 * m.
    #   sparse: edges <= 300 + 2 * 300 = 900 <= 9600 -> short teams (8 KW lanes, at most 64); free entries <= 600 * 8 = 4800 <=
    #           32 * 608 = 19 456 -> short residual teams.
    #   dense:  edges ~ 0.5 * 300 * 300 = 45 000 > 9600 -> a whole wave per descriptor; free entries ~ 0.9 * 600 * 64 = 34 560 >
    #           32 * 664 = 21 248 -> a whole wave per column.
    # k = 1 (KW = 1) and k = 3 (KW = 4) are where the two team shapes differ; test_layered_construction asserts the sides.
    "300+300 sparse": dict(widths=[300, 300], extra_free=8, team="short"),
    "300+300 dense": dict(widths=[300, 300], extra_free=64, feed=0.5, free_density=0.9, team="long"),
    # duplicate (row, column) entries on the diagonal, inside a chunk's block, in push descriptors and on free columns
    "duplicates": dict(widths=[40, 30, 300, 20], dup=True),
}
KS = (1, 3, 65)


def layered_case(name, p, kind):
    """The matrix of LAYERS[name], its dense image, a planted solution Y (65 vectors) with b = Y T, and 65 random int32 vectors"""
    opt = dict(LAYERS[name])
    widths, team = opt.pop("widths"), opt.pop("team", None)
    opt.setdefault("extra_free", 7)
    rng = np.random.default_rng(sum(map(ord, name)) * 7 + p % 1009 + (kind == "back"))
    T, piv, rowcol, prow, pcol, counts = layered(widths, p, rng, kind, **opt)
    Y = np.zeros((T.n, max(KS)), dtype=np.int64)
    Y[prow] = rng.integers(0, p, size=(len(prow), max(KS)))
    D = dense_of(T)
    return SimpleNamespace(T=T, piv=piv, rowcol=rowcol, prow=prow, pcol=pcol, counts=counts, widths=widths, team=team, D=D, Y=bal(Y, p),
                           B=bal(xT(Y, D, p), p), R=rand_int32(rng, (T.m, max(KS))))


def test_packing_rule():
    """pack() against plans worked out by hand from the rule"""
    want = {"255": (0, 4), "256": (1, 0), "257": (1, 0), "63": (0, 1), "64": (0, 1), "65": (0, 2), "63+2": (0, 2), "100+28+5": (0, 3),
            "65x1": (0, 2), "256+255+256": (2, 4), "300+10+300+64+64+1": (2, 4), "40+300+40": (1, 2), "300+300 sparse": (2, 0),
            "300+300 dense": (2, 0), "duplicates": (1, 3)}  # duplicates: 40 + 24 | 6, closed by the wide level | 20
    assert {name: pack(opt["widths"]) for name, opt in LAYERS.items()} == want
    assert pack([255, 2]) == (0, 5) and pack([]) == (0, 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p", PRIMES_B)
@pytest.mark.parametrize("name", list(LAYERS))
def test_layered_construction(name, p, kind):
    c = layered_case(name, p, kind)
    assert kahn_widths(c.T, c.rowcol) == list(c.widths)
    assert np.array_equal(sparse_xT(c.T, c.Y), c.B.astype(np.int64) % p)  # planted: y T = b, by a second route
    assert not c.Y[np.setdiff1d(np.arange(c.T.n), c.prow)].any()
    if c.team is not None:
        q = c.counts
        assert q.targets == 300
        assert (q.edges > 32 * q.targets) == (c.team == "long") and (q.nres > 32 * q.m) == (c.team == "long")
    if name == "duplicates":
        T = c.T
        nnz = int(T.p[T.n])
        rows = np.repeat(np.arange(T.n), np.diff(T.p))
        key, cnt = np.unique(rows * T.m + T.j[:nnz], return_counts=True)
        twice = key[cnt == 2]
        tr, tc = twice // T.m, twice % T.m
        colpiv = np.isin(tc, c.pcol)
        assert (cnt <= 2).all() and (c.rowcol[tr] == tc).any() and (colpiv & (c.rowcol[tr] != tc)).any() and (~colpiv).any()


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p", PRIMES_B)
@pytest.mark.parametrize("name", list(LAYERS))
def test_layered_plan_and_solution(S, name, p, kind):
    c = layered_case(name, p, kind)
    n, m = c.T.n, c.T.m
    idle = np.setdiff1d(np.arange(n), c.prow)
    with S.TriangularSolver(on_device(S, c.T), c.piv, kind) as ts:
        st = ts.stats()
        assert (st["n"], st["m"], st["rows"]) == (n, m, len(c.prow))
        assert st["levels"] == len(c.widths)
        assert (st["wide_panels"], st["chunks"]) == pack(c.widths)
        for k in KS:  # planted: the solution is y, nothing is left of b
            B = c.B[:, :k].copy()
            X, ok = ts.solve(B)
            assert ok.all() and not B.any() and np.array_equal(X, c.Y[:, :k]), k
        # random int32 b: zero residual on the pivot columns and zero x off the participating rows fix x; B = b - x T
        X65 = B65 = None
        for k in KS[::-1]:
            B = c.R[:, :k].copy()
            X, ok = ts.solve(B)
            if k == max(KS):
                X65, B65 = X, B
                res = bal(c.R.astype(np.int64) - xT(X, c.D, p), p)
                assert np.array_equal(B, res) and not B[c.pcol].any() and not X[idle].any()
            assert np.array_equal(X, X65[:, :k]) and np.array_equal(B, B65[:, :k]) and np.array_equal(ok, ~B65[:, :k].any(axis=0)), k


# ---- D: the diagonal of a row that repeats its pivot entry with unreduced values ----------------------------------------------------

# zp_reduce is exact for |x| <= min(3 * 2^51 * p, 2^62) (csrc/zp.hpp).  trsolve_create sums the entries of a row on its own pivot
# column -- the caller's raw ints, repeated entries included -- so the sum of the raw values leaves that domain once one row of
# p = 3 repeats a value near 2^31 more than 3 * 2^20 * p = 9 437 184 times; the entries are therefore reduced one by one.
# 9 437 185 is the first length past the domain; 16 777 244 is the first one at which the quotient of the raw sum
# N * (2^31 - 1) is 3 off, so that one reduction of it gives a wrong residue (found with the same double arithmetic on the CPU).
DIAG_V = 2**31 - 1
DIAG_LENGTHS = [3 * 2**20 * 3 + 1, 16777244]


@gpu
@pytest.mark.parametrize("N", DIAG_LENGTHS)
def test_diagonal_of_repeated_unreduced_entries(S, N):
    """One row, one column, p = 3: N entries 2^31 - 1 on the pivot column.  The diagonal is N * (2^31 - 1) mod 3 in Python integers
    (1 for the first length, -1 for the second).  Back solve: x = b / d for b in {1, -1}; forward solve: accepted when d = 1, and
    refused with the true value in the text otherwise."""
    p = 3
    assert N * DIAG_V > 3 * 2**51 * p >= (DIAG_LENGTHS[0] - 1) * DIAG_V
    d = int(bal(np.asarray([N * DIAG_V % p]), p)[0])
    assert d in (1, -1)
    T = S.CSR.from_arrays(1, 1, np.array([0, N], dtype=np.int64), np.zeros(N, dtype=np.int32), np.full(N, DIAG_V, dtype=np.int32), prime=p)
    piv = np.zeros(1, dtype=np.int32)
    with S.TriangularSolver(T, piv, "back") as ts:
        B = np.array([[1, -1]], dtype=np.int32)
        X, ok = ts.solve(B)
        assert ok.all() and not B.any()
        assert X.tolist() == [[d, -d]]  # d is its own inverse
    if d == 1:
        with S.TriangularSolver(T, piv, "forward") as ts:
            B = np.array([-1], dtype=np.int32)
            X, ok = ts.solve(B)
            assert ok and X.tolist() == [-1]
    else:
        with pytest.raises(S.SpasmError, match=r"the pivot of row 0 \(column 0\) is -1, not 1"):
            S.TriangularSolver(T, piv, "forward")
