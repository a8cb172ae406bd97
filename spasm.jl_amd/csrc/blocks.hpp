// blocks.hpp -- the connected components of the row/column graph of a CSR matrix and the split of the matrix into its blocks, on
// the device, laid out as the batch (batch.hpp) reads its input: one concatenated CSR, rows + 1 row pointers per block.
//
// Graph.  Vertices 0 .. n-1 are the rows, n .. n+m-1 the columns (n + m < 2^31).  Every STORED entry (i, j) is the edge (i, n+j),
// whatever its value: an explicit zero is an edge, a repeated (i, j) is the same edge twice (reference src/blocks.jl:43-47).
//
// Components.  parent[n+m] is a union-find forest in global memory, parent[v] = v at the start.  Four kernels, each a phase:
//   (a) k_blk_rows<BLK_MINCOL>   parent[n+j] = min(parent[n+j], i) for every entry: a column hangs under the smallest row that holds
//                                it (a real edge; a column without entries stays its own root).  One no-return atomic min per entry.
//   (b) k_blk_rows<BLK_UNITE>    unite(i, parent[n+j]) for every entry: the rows that share a column end in one tree.  Only row
//                                vertices are touched (the parent of a row is a row), the column words are read-only here.
//   (c) k_blk_flatten            parent[v] = find(v), and root[v] = (find(v) == v)
//   (d) an exclusive scan of root[] numbers the roots; k_blk_label gives every vertex the number of its root.
// The index split (n == m, below) runs one more phase between (b) and (c), in a launch of its own:
//   (t) k_blk_tie                unite(i, parent[n+i]) for every i: row i and column i end in one tree.
//
// The one hooking rule: unite(a, b) finds the two roots and hangs the LARGER root under the SMALLER one with
// atomicCAS(&parent[hi], hi, lo); when the CAS fails (hi is no longer a root) it starts again from what the CAS returned.  find()
// halves the path with atomic min.  So every value ever stored in parent[v] is <= v, and < v once v is not a root: all writes are
// atomic mins or a CAS from v to something smaller.  Three things follow.
//   Termination.  find() walks a strictly decreasing chain of ids, at most n + m steps, whatever it reads.  Every retry of unite()
//     has a strictly smaller max(a, b) than the one before: after a failed CAS both ends are below hi.  No loop waits for another
//     thread, so a wrong input cannot spin a kernel either: the loops are bounded by the ids, not by the data.
//   The root is the minimum.  By induction a root is the smallest vertex of its tree (true for single vertices and for the stars of
//     (a); a hook joins two trees under the smaller of their two minima).  After (b) the trees are the components, so the root of a
//     component is its smallest vertex: a row when the component holds one, else the lone column.
//   Order does not matter.  The final forest of (c) is parent[v] = min of v's component for every v: a function of the graph, not of
//     how the races of (a), (b) resolved (path halving writes ancestors only, and the min over everything ever written to parent[v]
//     in (c) is the root).  Numbers, maps and the split are deterministic functions of that forest (scans, STABLE radix sorts, and
//     copies to places computed from them).
//
// Stale reads are safe.  Reads of parent[] are relaxed device-scope atomic loads, writes relaxed device-scope read-modify-writes.
// parent[v] only decreases, and every value it ever held is an ancestor-or-self of v in the forest of that moment and stays in v's
// tree for good (trees only merge).  A reader that sees an OLD value therefore sees a vertex of the right tree with an id <= v: find
// continues from there and still ends at a vertex that was a root when it was read.  If that vertex has been hooked since, the CAS
// of unite (atomic at the L2, expected value = the vertex itself) fails and returns the newer parent: nothing is lost, the retry
// goes on below.  An edge is never dropped: unite returns only when both ends had the same root or its own CAS succeeded.  What
// one PHASE wrote is visible to the next because a kernel boundary lies between them; no fence is needed inside a kernel.
//
// Index split.  For a square matrix the graph gets the edge (i, n+i) for every i on top of the entries' edges: row i and column i
// count as ONE vertex, the index i.  The components are then sets S_b of indices, A is diag(A[S_0,S_0], A[S_1,S_1], ..) up to a
// SIMULTANEOUS permutation of rows and columns, and a similarity keeps the spectrum: chi_A = prod chi_{A[S_b,S_b]}.  (The free
// split pairs rows with columns as it likes: rank and determinant up to sign survive, the characteristic polynomial does not --
// the 3-cycle permutation matrix is three 1 x 1 blocks there and one 3 x 3 block here.)
//   Why (t) is a launch of its own.  (b) rests on "the column words are read-only here".  The tie WRITES column words: a column
//     without entries is its own root after (a), and unite(i, n+i) hooks it under the root of row i (n+i is the larger id).  After
//     the kernel boundary behind (b) every column word is either a row that holds the column (hence, by (b), a vertex of the tree
//     of every row that holds it) or the column itself.  In (t) the word parent[n+i] is read by thread i alone (no row ever gets a
//     column as parent: a hook puts the larger id under the smaller, and every column id is above every row id) and written by
//     thread i alone (the CAS of its own unite, from n+i to a row).  All other traffic of (t) is unite on row words, as in (b).
//   The three properties.  Every write of (t) is still an atomic min of find or a CAS from v to something smaller, so the chain
//     argument of Termination holds word for word (a failed CAS leaves both ends below hi).  The root is the minimum: the induction
//     is over hooks, and (t) adds hooks of the same kind only.  After (t) both ends of every edge of the extended graph lie in one
//     tree: an entry edge (i, n+j) because parent[n+j] is a row that (b) united with i (or became one of its tree in (t): trees
//     only merge), a tie edge because unite(i, parent[n+i]) returned.  So the trees are the components of the extended graph and
//     (c) leaves parent[v] = min of v's component: a function of the graph, not of the races of (a), (b), (t).  Stale reads: as
//     below, nothing in the argument looks at which kernel wrote a value.
//   Consequences.  Every component holds i together with n+i, so its smallest vertex is a row and row_block[i] == col_block[i].
//     The two stable sorts then see the same keys in the same order: block_rows == block_cols block for block, every block is
//     square, row_pos[i] == col_pos[i], and the blocks ascend by their smallest index.  There is no 1 x 0 or 0 x 1 block: an index
//     with neither row nor column entries is a 1 x 1 zero block.  Two handles of one matrix are byte-identical, as before.
//
// Numbering (the contract of Block.from_csr).  Blocks in ascending order of their smallest vertex = ascending root id, rows before
// columns; inside a block the rows and the columns keep their order in A.  A stable radix sort of (block number, index) for the rows
// and another for the columns gives block_rows / block_cols; k_blk_starts finds row_start[b] by a binary search in the sorted keys;
// row_pos = place in the sorted order - row_start[block].
//
// Split.  len[q + b] = length of the q-th row of block_rows (b its block) and 0 on the extra slot of every block; the exclusive scan
// of len is the concatenated row-pointer array P (global entry offsets).  k_blk_rows<BLK_COPY> writes J = col_pos[A.j], X = A.x, the
// entries of a row in A's order.
//
// Walking the entries (a, b, copy).  TEAM lanes per row (1, 8 or 64 by the average row length, the two-way split of spg_nseg taken
// one step further); a row longer than BLK_LONG is left to k_blk_long, one workgroup of 256 per such row: the rows were listed by
// phase (a) (their order in the list is a race and has no effect: (a) and (b) commute, the copy writes to computed places).
#pragma once
#include <hip/hip_runtime.h>
#include "common.hpp"

#define BLK_LONG 512   // entries: longer rows are walked by a workgroup

enum { BLK_MINCOL = 0, BLK_UNITE = 1, BLK_COPY = 2 };

struct BlkArgs {
    int n, m;
    const i64d *P;        // A: row pointers, columns, values
    const int *J;
    const int *X;
    int *parent;          // n + m
    int *nlong;           // rows longer than BLK_LONG: count, list
    int *longrows;
    // the copy
    const int *row_block, *row_pos, *col_pos;
    const i64d *row_start;
    const i64d *cP;       // concatenated row pointers
    int *cJ, *cX;
};

__device__ __forceinline__ int blk_ld(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void blk_min(int *p, int v) { (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of v as far as this thread can see; halves the path on the way (each step: parent[v] = min(parent[v], grandparent))
__device__ __forceinline__ int blk_find(int *parent, int v)
{
    int p = blk_ld(parent + v);
    while (p != v) {
        const int g = blk_ld(parent + p);
        if (g == p) return p;
        blk_min(parent + v, g);
        v = p;
        p = g;
    }
    return v;
}

__device__ __forceinline__ void blk_unite(int *parent, int a, int b)
{
    while (true) {
        a = blk_find(parent, a);
        b = blk_find(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        a = old; // < hi: hi was hooked by someone else in the meantime
        b = lo;
    }
}

// the entries e0 + tl, e0 + tl + step, .. of row i
template <int PH> __device__ __forceinline__ void blk_walk(const BlkArgs &a, int i, i64d e0, i64d e1, int tl, int step)
{
    if (PH == BLK_MINCOL) {
        for (i64d k = e0 + tl; k < e1; k += step) blk_min(a.parent + a.n + a.J[k], i);
    } else if (PH == BLK_UNITE) {
        int last = -1;
        for (i64d k = e0 + tl; k < e1; k += step) {
            const int r = blk_ld(a.parent + a.n + a.J[k]);
            if (r != i && r != last) blk_unite(a.parent, i, r);
            last = r;
        }
    } else {
        const int b = a.row_block[i];
        const i64d shift = a.cP[a.row_start[b] + a.row_pos[i] + b] - e0;
        for (i64d k = e0 + tl; k < e1; k += step) {
            a.cJ[k + shift] = a.col_pos[a.J[k]];
            a.cX[k + shift] = a.X[k];
        }
    }
}

template <int PH, int TEAM> __global__ __launch_bounds__(256) void k_blk_rows(BlkArgs a)
{
    const i64d t = ((i64d)blockIdx.x * blockDim.x + threadIdx.x) / TEAM;
    if (t >= a.n) return;
    const int i = (int)t, tl = threadIdx.x % TEAM;
    const i64d e0 = a.P[i], e1 = a.P[i + 1];
    if (e1 - e0 > BLK_LONG) {
        if (PH == BLK_MINCOL && tl == 0) a.longrows[atomicAdd(a.nlong, 1)] = i;
        return;
    }
    blk_walk<PH>(a, i, e0, e1, tl, TEAM);
}

template <int PH> __global__ __launch_bounds__(256) void k_blk_long(BlkArgs a)
{
    const int nl = *a.nlong;
    for (int q = blockIdx.x; q < nl; q += gridDim.x) {
        const int i = a.longrows[q];
        blk_walk<PH>(a, i, a.P[i], a.P[i + 1], threadIdx.x, 256);
    }
}

__global__ void k_blk_init(int nv, int *__restrict__ parent)
{
    const i64d v = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < nv) parent[v] = (int)v;
}

// (t): the tie of the index split, row i with column i (n == m); the only phase that writes a column word after (a)
__global__ void k_blk_tie(int n, int *parent)
{
    const i64d i = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    blk_unite(parent, (int)i, blk_ld(parent + n + i));
}

// (c): every vertex straight under its root; root[v] = 1 for the roots (no hook happens here, so a root stays one)
__global__ void k_blk_flatten(int nv, int *parent, int *__restrict__ root)
{
    const i64d v = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const int r = blk_find(parent, (int)v);
    blk_min(parent + v, r);
    root[v] = r == (int)v ? 1 : 0;
}

// (d): block of a vertex = number of its root; the sort's values (the indices) on the side
__global__ void k_blk_label(int n, int m, const int *__restrict__ parent, const int *__restrict__ num, int *__restrict__ row_block, int *__restrict__ col_block,
                            int *__restrict__ iota)
{
    const i64d v = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= (i64d)n + m) return;
    const int b = num[parent[v]];
    if (v < n) row_block[v] = b;
    else col_block[v - n] = b;
    if (v < (n > m ? n : m)) iota[v] = (int)v;
}

// start[b] = first place of the sorted keys that holds a key >= b, b = 0 .. nb (start[nb] = cnt)
__global__ void k_blk_starts(int nb, int cnt, const int *__restrict__ key, i64d *__restrict__ start)
{
    const i64d b = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    if (b > nb) return;
    int lo = 0, hi = cnt;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (key[mid] < (int)b) lo = mid + 1;
        else hi = mid;
    }
    start[b] = lo;
}

// pos[member[q]] = q - start[key[q]]; with P (rows only): len[q + key[q]] = length of that row of A (len was zeroed)
__global__ void k_blk_pos(int cnt, const int *__restrict__ key, const int *__restrict__ member, const i64d *__restrict__ start, int *__restrict__ pos,
                          const i64d *__restrict__ P, i64d *__restrict__ len)
{
    const i64d q = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= cnt) return;
    const int b = key[q], i = member[q];
    pos[i] = (int)(q - start[b]);
    if (P) len[q + b] = P[i + 1] - P[i];
}

// entries of every block, from the ends of its row pointers
__global__ void k_blk_nnz(int nb, const i64d *__restrict__ row_start, const i64d *__restrict__ cP, i64d *__restrict__ nnz)
{
    const i64d b = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    nnz[b] = cP[row_start[b + 1] + b] - cP[row_start[b] + b];
}
