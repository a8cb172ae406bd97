"""Block-diagonal driver: mirror of SpaSM.jl's src/blocks.jl over the C ABI.

`Block(A)` splits a CSR into the connected components of its row/column graph (reference
src/blocks.jl:35-105); `echelonize`, `rank`, `kernel` then run block by block (:107-139) and
`to_csr` stitches a block matrix back together (:142-170).  Blocks are independent units: with one
process per GPU, `owner=(rank, world)` makes a process work only on its share (zero communication).

`api.DeviceBlocks(A)` is the same split done on the device (csrc/blocks.hpp); `echelonize`, `rank`, `kernel` take it in place of
a Block and run all blocks as one batch whose input never leaves the device.  `solve(block, B)` is the reference's
sparse_triangular_solve(block::Block{LU{F}}, B) (src/blocks.jl:172-226) without the factorization in between: X with X * A == B.
"""
import numpy as np

from . import api


class Block:
    """blocks[b] with the maps row2block / col2block = (block, position, 0-based) and their inverses (src/blocks.jl:1-7)."""

    def __init__(self, blocks, row2block, col2block, block2row, block2col, index=False):
        self.index = index  # True: split by index (row i and column i are one vertex), see from_csr
        self.blocks = blocks
        self.row2block = row2block
        self.col2block = col2block
        self.block2row = block2row
        self.block2col = block2col

    def __len__(self):
        return len(self.blocks)

    @property
    def shape(self):  # Base.size(block), src/blocks.jl:11
        return (len(self.row2block), len(self.col2block))

    @classmethod
    def from_csr(cls, A, device=False, index=False):
        """Block(A::CSR): union-find over rows and columns joined by the non-zeros (src/blocks.jl:35-105).
        Blocks are numbered by their smallest member in (rows, then columns) order.  device=True: the same Block, found and
        split on the device (api.DeviceBlocks).
        index=True (a square A): row i and column i are one vertex, i.e. the graph gets the edge row i - column i for every i.  The
        blocks are then A[S, S] for the components S of the index graph, A is block diagonal up to a SIMULTANEOUS permutation of rows
        and columns, and charpoly(block) is the product of the blocks' characteristic polynomials.  On the host this is a plain
        union-find in Python (the larger root goes under the smaller), independent of the device code."""
        n, m = A.shape
        if index and n != m:
            raise ValueError(f"not square ({n} x {m})")
        if device:
            with api.DeviceBlocks(A, index=index) as D:
                B = D.to_block()
            return cls(B.blocks, B.row2block, B.col2block, B.block2row, B.block2col, index=index)
        nz = api.nnz(A)
        p, j, x = A.p, A.j[:nz], A.x[:nz]
        if index:
            parent = list(range(n + m))

            def find(v):
                while parent[v] != v:
                    parent[v] = parent[parent[v]]
                    v = parent[v]
                return v

            def unite(a, b):
                a, b = find(a), find(b)
                if a != b:
                    parent[max(a, b)] = min(a, b)

            pl, jl = [int(v) for v in p[: n + 1]], j.tolist()
            for i in range(n):
                for k in range(pl[i], pl[i + 1]):
                    unite(i, n + jl[k])  # every stored entry, whatever its value
                unite(i, n + i)  # the tie
            roots = [find(v) for v in range(n + m)]
            number = {r: b for b, r in enumerate(sorted(set(roots)))}
            ncomp, lab = len(number), np.array([number[r] for r in roots], dtype=np.int64)
        else:
            import scipy.sparse as sp
            from scipy.sparse.csgraph import connected_components

            rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(p))
            G = sp.coo_matrix((np.ones(nz, dtype=np.int8), (rows, j.astype(np.int64) + n)), shape=(n + m, n + m))
            ncomp, lab = connected_components(G, directed=False)
        first = np.full(ncomp, n + m, dtype=np.int64)
        np.minimum.at(first, lab, np.arange(n + m))
        renum = np.empty(ncomp, dtype=np.int64)
        renum[np.argsort(first, kind="stable")] = np.arange(ncomp)
        lab = renum[lab]
        block2row = [[] for _ in range(ncomp)]
        block2col = [[] for _ in range(ncomp)]
        row2block, col2block = [], []
        for i in range(n):
            b = int(lab[i])
            row2block.append((b, len(block2row[b])))
            block2row[b].append(i)
        for c in range(m):
            b = int(lab[n + c])
            col2block.append((b, len(block2col[b])))
            block2col[b].append(c)
        colpos = np.array([q for _, q in col2block], dtype=np.int32)
        blocks = []
        for b in range(ncomp):
            rws = block2row[b]
            lens = np.array([int(p[i + 1] - p[i]) for i in rws], dtype=np.int64)
            sp_ = np.concatenate([[0], np.cumsum(lens)]) if rws else np.zeros(1, dtype=np.int64)
            idx = np.concatenate([np.arange(p[i], p[i + 1]) for i in rws]) if rws and sp_[-1] else np.zeros(0, dtype=np.int64)
            blocks.append(api.CSR.from_arrays(len(rws), len(block2col[b]), sp_, colpos[j[idx]] if len(idx) else [], x[idx] if len(idx) else [], prime=A.prime))
        return cls(blocks, row2block, col2block, block2row, block2col, index=index)

    def to_csr(self):
        """CSR(block::Block{CSR}) (src/blocks.jl:142-170)."""
        n, m = self.shape
        present = [b for b in self.blocks if b is not None]
        prime = present[0].prime if present else api.prime0
        rows = []
        cache = [b.rows() if b is not None else [] for b in self.blocks]
        for i in range(n):
            b, sub = self.row2block[i]
            rows.append([(self.block2col[b][c], v) for c, v in cache[b][sub]])
        return api.CSR.from_rows(rows, m, prime=prime)


def _device(block, owner):
    """True for an api.DeviceBlocks (one handle, one process: no share of it can be given away)"""
    if not isinstance(block, api.DeviceBlocks):
        return False
    if owner is not None:
        raise ValueError("owner= cannot be combined with DeviceBlocks: a handle belongs to one process")
    return True


def _mine(block, owner):
    """indices of the blocks of the caller's share (owner=(rank, world): b % world == rank) that are present"""
    return [b for b, X in enumerate(block.blocks) if X is not None and (owner is None or b % owner[1] == owner[0])]


def echelonize(block, owner=None, batched=False, **kwargs):
    """echelonize(block::Block{CSR}) (src/blocks.jl:107-115).  owner=(rank, world): only blocks b % world == rank.
    batched=True: the blocks of the share go through ONE api.echelonize_batch call instead of a loop over api.echelonize (small
    blocks are then eliminated inside LDS with canonical pivot columns, whatever the pivot-search options say).
    A DeviceBlocks in place of the Block: what Block.from_csr(A) gives with batched=True, from the blocks on the device."""
    if _device(block, owner):
        return Block(block.echelonize(**kwargs), *block.block_maps())
    lus = [None] * len(block.blocks)
    mine = _mine(block, owner)
    if batched:
        for b, lu in zip(mine, api.echelonize_batch([block.blocks[b] for b in mine], **kwargs)):
            lus[b] = lu
    else:
        for b in mine:
            lus[b] = api.echelonize(block.blocks[b], **kwargs)
    return Block(lus, block.row2block, block.col2block, block.block2row, block.block2col)


def rank(block, owner=None, batched=False, **kwargs):
    """rank(block) = sum of the ranks (src/blocks.jl:117) over the blocks of the share.  batched=True: one api.rank_batch call
    for the blocks that are still matrices.  A DeviceBlocks: the ranks of its blocks, from the device."""
    if _device(block, owner):
        return sum(block.rank(**kwargs))
    mine = _mine(block, owner)
    if batched:
        mats = [block.blocks[b] for b in mine if isinstance(block.blocks[b], api.CSR)]
        rest = [block.blocks[b] for b in mine if not isinstance(block.blocks[b], api.CSR)]
        return sum(api.rank_batch(mats, **kwargs)) + sum(api.rank(X) for X in rest)
    return sum(api.rank(block.blocks[b], **kwargs) for b in mine)


def kernel(block, owner=None, batched=False, **kwargs):
    """kernel(block::Block{LU}) (src/blocks.jl:119-137): per-block kernels, rows numbered block after block; a block outside the
    share (or absent) contributes no rows.  batched=True on a Block of matrices: one api.kernel_batch call for the share.
    A DeviceBlocks: the kernels of its blocks, from the device."""
    if _device(block, owner):
        ks = block.kernel(**kwargs)
        _, col2block, _, block2col = block.block_maps()
        return _kernel_block(ks, col2block, block2col)
    ks = [None] * len(block.blocks)
    mine = _mine(block, owner)
    if batched and all(isinstance(block.blocks[b], api.CSR) for b in mine):
        for b, k in zip(mine, api.kernel_batch([block.blocks[b] for b in mine], **kwargs)):
            ks[b] = k
    else:
        if block.blocks and any(isinstance(block.blocks[b], api.CSR) for b in mine):
            block = echelonize(block, owner=owner, batched=batched, **kwargs)
        for b in mine:
            ks[b] = api.kernel(block.blocks[b])
    return _kernel_block(ks, block.col2block, block.block2col)


def solve(block, B):
    """(X, ok) with X * A == B row by row for the matrix A the block was split from (reference src/blocks.jl:172-226, from the
    matrices instead of their LUs).  A DeviceBlocks goes to the device entry (api.DeviceBlocks.solve).  A host Block of matrices
    deals the entries of B to the blocks by col2block, solves all blocks with ONE api.solve_batch call and places each block's
    solution on the block's rows through block2row; a row of B is solvable iff it is in every block, and an entry that is non-zero
    mod p on an empty column of A (a block without rows) makes its row unsolvable."""
    if isinstance(block, api.DeviceBlocks):
        return block.solve(B)
    if not isinstance(B, api.CSR):
        raise TypeError("a CSR expected")
    n, m = block.shape
    if B.m != m:
        raise ValueError("B needs as many columns as the block matrix")
    prime = B.prime
    K = B.n
    nb = len(block.blocks)
    pieces = [dict() for _ in range(nb)]  # block -> {row of B: [(position, value), ...]}, rows in ascending order
    for k, row in enumerate(B.rows()):
        p0, p1 = int(B.p[k]), int(B.p[k + 1])
        for c, v in zip(B.j[p0:p1].tolist(), B.x[p0:p1].tolist()):
            b, pos = block.col2block[c]
            pieces[b].setdefault(k, []).append((pos, v))
    used = [b for b in range(nb) if pieces[b]]
    for b in used:
        if not isinstance(block.blocks[b], api.CSR):
            raise TypeError("a Block of CSR expected")
    rhs = [api.CSR.from_rows([pieces[b][k] for k in sorted(pieces[b])], block.blocks[b].m, prime=prime) for b in used]
    xs, oks = api.solve_batch([block.blocks[b] for b in used], rhs)
    ok = np.ones(K, dtype=np.bool_)
    rows = [[] for _ in range(K)]
    for b, Xb, okb in zip(used, xs, oks):
        for t, (k, xr) in enumerate(zip(sorted(pieces[b]), Xb.rows())):
            ok[k] &= bool(okb[t])
            rows[k] += [(block.block2row[b][c], v) for c, v in xr]
    X = api.CSR.from_rows([sorted(r) if ok[k] else [] for k, r in enumerate(rows)], n, prime=prime)
    return X, ok


def solver(block):
    """The resident solver of a split matrix: api.BatchSolver.from_blocks for a DeviceBlocks (the blocks are factored once, on the
    device; solver.solve(B) then returns what solve(block, B) returns without eliminating them again)."""
    if not isinstance(block, api.DeviceBlocks):
        raise TypeError("a DeviceBlocks expected: the blocks of a resident solver live on the device")
    return block.solver()


def _kernel_block(ks, col2block, block2col):
    """the Block of per-block kernels: rows numbered block after block"""
    block2row, row2block, r = [], [], 0
    for b, k in enumerate(ks):
        kn = k.n if k is not None else 0
        block2row.append(list(range(r, r + kn)))
        row2block += [(b, i) for i in range(kn)]
        r += kn
    return Block(ks, row2block, col2block, block2row, block2col)


def det(block):
    """The determinant mod p of the matrix the block was split from, as a balanced residue.  A DeviceBlocks goes to the device entry
    (api.DeviceBlocks.det).  A host Block of matrices: 0 when a block is not square, otherwise ONE api.det_batch call for the
    blocks, their product, and the parities of the row and the column permutation that put the blocks on the diagonal."""
    if isinstance(block, api.DeviceBlocks):
        return block.det()
    n, m = block.shape
    if n != m:
        raise ValueError("a square matrix expected")
    for X in block.blocks:
        if not isinstance(X, api.CSR):
            raise TypeError("a Block of CSR expected")
    if any(X.n != X.m for X in block.blocks):
        return 0
    if not block.blocks:
        return 1
    p = block.blocks[0].prime
    value = 1
    for d in api.det_batch(block.blocks).tolist():
        value = value * d % p
    start = np.concatenate(([0], np.cumsum([X.n for X in block.blocks])))
    for to_block in (block.row2block, block.col2block):
        perm = [int(start[b]) + pos for b, pos in to_block]
        seen, cycles = [False] * n, 0
        for i in range(n):
            if not seen[i]:
                cycles += 1
                while not seen[i]:
                    seen[i] = True
                    i = perm[i]
        if (n - cycles) % 2:
            value = -value % p
    return int(api.balanced(value, p))


def charpoly(block):
    """The n + 1 coefficients of det(x * I - A) mod p of the matrix the block was split from.  Only an INDEX split keeps the
    spectrum: a DeviceBlocks made with index=True goes to the device entry (api.DeviceBlocks.charpoly); a host Block made with
    Block.from_csr(A, index=True) takes ONE api.charpoly_batch call for its blocks and api.poly_product for their product.  A Block
    without index is refused."""
    if isinstance(block, api.DeviceBlocks):
        return block.charpoly()
    if not getattr(block, "index", False):
        raise ValueError("the Block is not an index split (Block.from_csr(A, index=True)): its blocks do not carry the spectrum")
    for X in block.blocks:
        if not isinstance(X, api.CSR):
            raise TypeError("a Block of CSR expected")
    if not block.blocks:
        return np.ones(1, dtype=np.int32)
    return api.poly_product(api.charpoly_batch(block.blocks), block.blocks[0].prime)
