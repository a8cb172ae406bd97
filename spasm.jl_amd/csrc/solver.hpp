// solver.hpp -- X * A = B for many small matrices with A factored ONCE: the resident operator behind spasm_amd_solver_*.  The
// companion of solve_batch.hpp; it shares that file's limits, classes and elimination (batch_eliminate) and returns what it returns.
//
// k_solve_elim eliminates the transposed image [A^T | b^T] (m image rows = the columns of A, n candidate columns = the rows of A)
// on every call.  Let T be the m x m transform the elimination applies to the image rows, pr_1 .. pr_r the pivot image rows (columns
// of A, the set J), c_1 < .. < c_r the pivot columns (the canonical row basis of A) and pinv_k the inverse of the k-th pivot.  A
// right-hand side b, as a column, ends as T * b, and k_solve_elim reads ok and x off that column.
//
// Only pivot rows are ever subtracted from other rows, and a pivot row only receives multiples of other pivot rows, so every row of
// T is e_i plus a combination of the unit vectors of J.  With G = T[:, J] (m x r) and y = G * b_J therefore
//   (T * b)_i = y_i + b_i  for i outside J,      (T * b)_i = y_i  for i in J (e_i is the column of G that belongs to i),
//   ok iff y_i + b_i == 0 for every i outside J,  x[c_k] = y[pr_k] * pinv_k, every other x = 0.
// pinv_k is folded into row pr_k of G when it is written, so y[pr_k] IS x[c_k].  Every value is the canonical balanced residue, so
// the row of X is bit for bit the one k_solve_elim packs.
//
// k_solver_factor (create) is the sibling of k_solve_elim: it scatters [A^T | a slab of the m identity columns], eliminates with the
// first n columns as candidates, and what is left in identity column t is column t of T.  The columns with t in J go to G (column
// k of G, for pr_k = t, at G[goff + k * m ..], m words); the slabs of a system elect the same pivots (the election never looks right
// of column n), so each writes its own columns and the first one writes the pivots and the rank.  No atomics, one writer per word.
//
// k_solver_apply: one workgroup per (system, slab of right-hand sides).  LDS: G with row stride ldg, then q vectors of m + r words
// (a right-hand side scattered densely, and its entries on the pivot rows gathered in k order).  m * r + m <= m * (n + 1) <=
// BATCH_LIMIT, so G and one vector always fit the largest class.  A group of >= m threads (whole waves) owns one right-hand side;
// thread i forms y_i = sum_k G[i][k] * b[pr_k] over the k with b[pr_k] != 0 (the entry is the same for the whole wave: a uniform
// skip), lazily as zp.hpp's ZpAcc: at most r < 182 terms, |term| <= halfp + 256 < 2^15.1 in i32 for p < 2^16 and < 2^31.1 in i64
// otherwise, far inside either accumulator for every prime.
//
// Row stride of G.  Lane i reads word i * ldg + k for one k at a time: the walk down a column that batch.hpp describes, conflict-free
// over the 32 banks of a half wave for odd ldg.  ldg = r for odd r, r + 1 when the padded operator and one vector still fit the
// largest class, else r.  Staging writes the same pattern (lanes along a column of G, which global memory holds contiguously).
#pragma once
#include <hip/hip_runtime.h>
#include "solve_batch.hpp"

struct SolverFactorDesc {
    i64d row0;    // P[row0 .. row0 + n]: the row pointers of A
    i64d goff;    // G of the system starts here; column k at goff + k * m
    i64d pivoff;  // pivrow / pivcol of the system start here
    int sys;      // rank[sys]
    int n, m, ld;
    int t0, w;    // the slab: identity columns t0 .. t0 + w - 1
    ZpField F;
};

struct SolverFactorArgs {
    const SolverFactorDesc *desc;
    const int *items;
    const i64d *P;             // A: concatenated CSR
    const int *J;
    const int *X;
    int cap, bw, rmax;         // LDS layout of the class, as in BatchArgs
    int *G;
    int *pivrow, *pivcol;
    int *rank;
};

template <int BS>
__global__ __launch_bounds__(BS) void k_solver_factor(SolverFactorArgs a)
{
    extern __shared__ int s_factor[];
    constexpr int NW = BS / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SolverFactorDesc d = a.desc[a.items[blockIdx.x]];
    const ZpField F = d.F;
    const int n = d.n, m = d.m, ld = d.ld, W = d.n + d.w;
    const BatchLds L(s_factor, a.cap, a.bw, a.rmax, false);
    int *img = L.img;

    batch_lds_clear<BS>(L, m * ld, a.bw);
    __syncthreads();
    batch_load_rows<BS, true>(F, img, ld, n, m, a.P + d.row0, a.J, a.X);   // (a row of A holds at most m entries)
    for (int t = tid; t < d.w; t += BS) img[(d.t0 + t) * ld + n + t] = 1;
    __syncthreads();

    const int r = batch_eliminate<BS, false>(F, L, ld, m, n, W, false, nullptr);

    // ---- one wave per identity column of the slab that belongs to a pivot row: column k of G
    for (int t = wave; t < d.w; t += NW) {
        const int row = d.t0 + t;
        if (!((L.rowflag[row >> 5] >> (row & 31)) & 1u)) continue;
        int k = -1;
        for (int k0 = 0; k0 < r && k < 0; k0 += 64) {
            const int kk = k0 + lane;
            const unsigned long long b = __ballot(kk < r && L.pivrow[kk] == row);
            if (b) k = k0 + (__ffsll((long long)b) - 1);
        }
        if (k < 0) continue; // (cannot happen: the flag is set with the list)
        int *g = a.G + d.goff + (i64d)k * m;
        const int col = n + t;
        for (int i = lane; i < m; i += 64)
            if (!((L.rowflag[i >> 5] >> (i & 31)) & 1u)) g[i] = img[i * ld + col];
        for (int kk = lane; kk < r; kk += 64) {
            const int pr = L.pivrow[kk];
            const int x = img[pr * ld + col];
            g[pr] = x == 0 ? 0 : zp_mul(F, x, L.pinv[kk]);
        }
    }
    if (d.t0 == 0) {
        for (int k = tid; k < r; k += BS) {
            a.pivrow[d.pivoff + k] = L.pivrow[k];
            a.pivcol[d.pivoff + k] = L.pivcol[k];
        }
        if (tid == 0) a.rank[d.sys] = r;
    }
}

struct SolverApplyDesc {
    i64d goff;    // G of the system
    i64d pivoff;  // its pivrow / pivcol
    i64d brow0;   // BP[brow0 .. brow0 + w]: the row pointers of the right-hand sides of this slab
    i64d slice;   // its slice of the entry scratch (int2): w * (r + 1)
    i64d slot0;   // the slot of its first right-hand side in ok / cnt / src
    int m, r, ldg;
    int w;        // right-hand sides of the slab
    int q;        // how many of them LDS holds at a time
    ZpField F;
};

struct SolverApplyArgs {
    const SolverApplyDesc *desc;
    const int *items;
    const int *G;
    const int *pivrow, *pivcol;
    const i64d *BP;            // right-hand sides: concatenated CSR
    const int *BJ;
    const int *BX;
    int cap, bw, rmax;         // LDS layout of the class, as in BatchArgs
    int2 *scratch;
    int *cnt;
    i64d *src;
    unsigned char *ok;
};

// y_i = sum over the pivots with a non-zero right-hand-side entry of G[i][k] * bJ[k]; g = row i of G
template <bool SMALL> __device__ inline int solver_dot(const ZpField &F, const int *g, const int *bJ, int r)
{
    typename ZpAcc<SMALL>::type acc = 0;
    for (int k = 0; k < r; k++) {
        const int b = bJ[k];
        if (b != 0) acc += ZpAcc<SMALL>::mul_lazy(F, g[k], b);
    }
    return zp_reduce(F, (int64_t)acc);
}

template <int BS>
__global__ __launch_bounds__(BS) void k_solver_apply(SolverApplyArgs a)
{
    extern __shared__ int s_apply[];
    const int tid = threadIdx.x, lane = tid & 63;
    const SolverApplyDesc d = a.desc[a.items[blockIdx.x]];
    const ZpField F = d.F;
    const int m = d.m, r = d.r, ldg = d.ldg;
    const BatchLds L(s_apply, a.cap, a.bw, a.rmax, false);
    int *G = L.img, *vec = G + m * ldg, *bad = L.wmin;

    // ---- stage the operator: G (global: column by column), the pivots, the bitset of the pivot rows
    for (int e = tid; e < m * r; e += BS) {
        const int k = e / m, i = e - k * m;
        G[i * ldg + k] = a.G[d.goff + e];
    }
    for (int k = tid; k < r; k += BS) {
        L.pivrow[k] = a.pivrow[d.pivoff + k];
        L.pivcol[k] = a.pivcol[d.pivoff + k];
    }
    __syncthreads();
    for (int w = tid; w * 32 < m; w += BS) {
        unsigned f = 0;
        for (int k = 0; k < r; k++) {
            const int pr = L.pivrow[k];
            if ((pr >> 5) == w) f |= 1u << (pr & 31);
        }
        L.rowflag[w] = f;
    }

    // ---- groups of whole waves, one right-hand side each; a system with more than BS image rows is one group that strides
    const int mp = (m + 63) & ~63;
    const bool split = mp <= BS;
    const int Q = split ? min(d.q, BS / mp) : 1;
    const int q = split ? tid / mp : 0, i0 = split ? tid - q * mp : tid, step = split ? mp : BS;
    int *b = vec + (q < Q ? q : 0) * (m + r), *bJ = b + m;
    for (int g0 = 0; g0 < d.w; g0 += Q) {
        const int t = g0 + q;
        const bool on = q < Q && t < d.w;
        if (on) {
            for (int i = i0; i < m; i += step) b[i] = 0;
            if (i0 == 0) bad[q] = 0;
        }
        __syncthreads();
        if (on) {
            const i64d e0 = a.BP[d.brow0 + t], e1 = a.BP[d.brow0 + t + 1];
            for (i64d e = e0 + i0; e < e1; e += step) b[a.BJ[e]] = zp_reduce(F, (int64_t)a.BX[e]);
        }
        __syncthreads();
        if (on)
            for (int k = i0; k < r; k += step) bJ[k] = b[L.pivrow[k]];
        __syncthreads();
        if (on)
            for (int i = i0; i < m; i += step) {
                const int y = F.small ? solver_dot<true>(F, G + i * ldg, bJ, r) : solver_dot<false>(F, G + i * ldg, bJ, r);
                if ((L.rowflag[i >> 5] >> (i & 31)) & 1u) b[i] = y;
                else if (zp_add(F, y, b[i]) != 0) bad[q] = 1;
            }
        __syncthreads();
        // ---- the first wave of the group: the row of X, in k order
        if (on && i0 < 64) {
            const bool nosol = bad[q] != 0;
            const i64d at = d.slice + (i64d)t * (r + 1);
            int2 *dst = a.scratch + at;
            int count = 0;
            for (int k0 = 0; k0 < r && !nosol; k0 += 64) {
                const int k = k0 + lane;
                int v = 0, pc = 0;
                if (k < r) {
                    pc = L.pivcol[k];
                    v = b[L.pivrow[k]];
                }
                batch_append(dst, count, pc, v);
            }
            if (lane == 0) {
                a.cnt[d.slot0 + t] = count;
                a.src[d.slot0 + t] = at;
                a.ok[d.slot0 + t] = nosol ? 0 : 1;
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// The dense apply: the same operator against right-hand sides that are COLUMNS of a dense row-major array B (M x K, leading
// dimension ldb), with the solutions as columns of X (N x K, ldx): the layout of spmv.hpp and trsolve.hpp, so that the three
// compose on one stream.  One workgroup per (system, slab of columns); nothing is scattered, appended, scanned or packed.
//
// Image row i of the system is row colmap[brow + i] of B and row j of the system is row rowmap[xrow + j] of X (a NULL map: the
// offset alone).  The product y = G * b_J for T = SOLVER_DENSE_T columns at a time is a small GEMM, (m x r) * (r x T): the r x T
// tile of b_J lies in LDS, k-major, and is read as a broadcast (two 16-byte reads per k); thread e walks its row of G once per k
// and keeps T lazy accumulators (ZpAcc, at most r <= 180 terms, the bounds above), so a word of G is read once per T columns.
// There is no skip on zero entries: a dense right-hand side is taken to be dense.
//
// Work items.  perm[0 .. r) = the pivot rows in k order, perm[r .. m) = the other image rows ascending; a group of >= m threads
// (whole waves; one group that strides when m exceeds the workgroup) owns a tile of columns, item e = row perm[e].  r never exceeds
// the group (r <= m, and r < cap / bs when m > bs), so a thread holds at most one pivot row: its T values of y wait in registers
// for the barrier after which the tile is no longer read, and then replace row k of the tile: x[c_k] = y[pr_k].  An item e >= r
// reads its own T contiguous words of B and tests y + b == 0; a failure sets the column's bit in the group's LDS word.
//
// Memory.  The contiguous axis of B and X is the column index.  Staging the tile: lanes along (k, t), t fastest, so 8 lanes read
// 32 contiguous bytes of one row of B.  The test: one thread reads T contiguous words of its row.  The store: thread j writes T
// contiguous words of row j of X, for all n rows of the system (the pivots' values, found by a binary search of j in the ascending
// pivcol, zeros everywhere else and in a column without solution).  One writer per word of X.
//
// ok.  A list handle: the workgroup writes ok[okoff + v].  A blocks handle: ok[v] is the AND over the blocks, so a failing
// workgroup sets flag[v] with a vector atomicOr and k_solver_dense_finish, launched after, writes ok[v] and zeroes column v of X.
// Systems without rows, columns or rank run the same code with r = 0 (n = 0: nothing to store; m = 0: nothing to test) and use
// no LDS beyond the group's word.
//
// LDS: G (row stride ldg, odd where it fits: the column walk above), perm (m words), q tiles of r * T words, each part rounded
// up to 16 bytes.  m * r + m <= m * (n + 1) <= BATCH_LIMIT and r * T <= 1440, so one tile always fits the largest class.
#define SOLVER_DENSE_T 8

struct SolverDenseDesc {
    i64d goff;    // G of the system
    i64d pivoff;  // its pivrow / pivcol
    i64d brow;    // its image rows in colmap (or in B)
    i64d xrow;    // its rows in rowmap (or in X)
    i64d okoff;   // ok[okoff + v] (a list handle)
    int n, m, r, ldg;
    int v0, w;    // the slab: columns v0 .. v0 + w - 1
    int q;        // tiles of T columns in flight
    ZpField F;
};

struct SolverDenseArgs {
    const SolverDenseDesc *desc;
    const int *items;
    const int *G;
    const int *pivrow, *pivcol;
    int cap, bw, rmax;         // LDS layout of the class, as in BatchArgs
    const int *B;
    i64d ldb;
    int *X;
    i64d ldx;
    const int *colmap, *rowmap;
    unsigned char *ok;         // a list handle
    unsigned *flag;            // a blocks handle: K words, cleared before the launch
};

// y[t] = sum_k g[k] * tile[k][t], reduced; g = a row of G
template <bool SMALL> __device__ inline void solver_dense_dot(const ZpField &F, const int *g, const int4 *tile, int r, int (&y)[SOLVER_DENSE_T])
{
    typename ZpAcc<SMALL>::type acc[SOLVER_DENSE_T];
#pragma unroll
    for (int t = 0; t < SOLVER_DENSE_T; t++) acc[t] = 0;
    for (int k = 0; k < r; k++) {
        const int gk = g[k];
        const int4 b0 = tile[2 * k], b1 = tile[2 * k + 1];
        acc[0] += ZpAcc<SMALL>::mul_lazy(F, gk, b0.x);
        acc[1] += ZpAcc<SMALL>::mul_lazy(F, gk, b0.y);
        acc[2] += ZpAcc<SMALL>::mul_lazy(F, gk, b0.z);
        acc[3] += ZpAcc<SMALL>::mul_lazy(F, gk, b0.w);
        acc[4] += ZpAcc<SMALL>::mul_lazy(F, gk, b1.x);
        acc[5] += ZpAcc<SMALL>::mul_lazy(F, gk, b1.y);
        acc[6] += ZpAcc<SMALL>::mul_lazy(F, gk, b1.z);
        acc[7] += ZpAcc<SMALL>::mul_lazy(F, gk, b1.w);
    }
#pragma unroll
    for (int t = 0; t < SOLVER_DENSE_T; t++) y[t] = zp_reduce(F, (int64_t)acc[t]);
}

template <int BS>
__global__ __launch_bounds__(BS) void k_solver_apply_dense(SolverDenseArgs a)
{
    extern __shared__ int s_dense[];
    static_assert(SOLVER_DENSE_T == 8, "solver_dense_dot is written out for 8 columns");
    constexpr int T = SOLVER_DENSE_T;
    const int tid = threadIdx.x, lane = tid & 63;
    const SolverDenseDesc d = a.desc[a.items[blockIdx.x]];
    const ZpField F = d.F;
    const int n = d.n, m = d.m, r = d.r, ldg = d.ldg;
    const BatchLds L(s_dense, a.cap, a.bw, a.rmax, false);
    int *G = L.img, *perm = G + ((m * ldg + 3) & ~3), *tiles = perm + ((m + 3) & ~3), *bad = L.wmin;
    unsigned *woff = L.rowflag + a.bw;   // (the words of colflag, which an apply does not keep)

    // ---- stage the operator: G (global: column by column), the pivots, the bitset of the pivot rows.  Without rank there is no
    // operator and no order to keep: item e is row e, LDS is not touched, and m is not bounded by the class (a system without rows).
    if (r > 0) {
        for (int e = tid; e < m * r; e += BS) {
            const int k = e / m, i = e - k * m;
            G[i * ldg + k] = a.G[d.goff + e];
        }
        for (int k = tid; k < r; k += BS) {
            const int pr = a.pivrow[d.pivoff + k];
            L.pivrow[k] = pr;
            L.pivcol[k] = a.pivcol[d.pivoff + k];
            perm[k] = pr;
        }
        __syncthreads();
        for (int w = tid; w * 32 < m; w += BS) {
            unsigned f = 0;
            for (int k = 0; k < r; k++) {
                const int pr = L.pivrow[k];
                if ((pr >> 5) == w) f |= 1u << (pr & 31);
            }
            L.rowflag[w] = f;
        }
        __syncthreads();
        // ---- woff[w] = pivot rows before word w (the first wave scans), then the other rows behind the pivots, ascending
        if (tid < 64) {
            int carry = 0;
            for (int w0 = 0; w0 * 32 < m; w0 += 64) {
                const int w = w0 + lane;
                const int c = w * 32 < m ? __popc(L.rowflag[w]) : 0;
                int s = c;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int up = __shfl_up(s, o);
                    if (lane >= o) s += up;
                }
                if (w * 32 < m) woff[w] = (unsigned)(carry + s - c);
                carry += __shfl(s, 63);
            }
        }
        __syncthreads();
        for (int i = tid; i < m; i += BS) {
            const unsigned f = L.rowflag[i >> 5];
            if (!((f >> (i & 31)) & 1u)) perm[r + i - (int)woff[i >> 5] - __popc(f & ((1u << (i & 31)) - 1u))] = i;
        }
    }

    // ---- groups of whole waves, one tile of T columns each; a system with more than BS image rows is one group that strides
    const int mp = m > 64 ? (m + 63) & ~63 : 64;
    const bool split = mp <= BS;
    const int Q = split ? min(d.q, BS / mp) : 1;
    const int q = split ? tid / mp : 0, i0 = split ? tid - q * mp : tid, step = split ? mp : BS;
    int *tile = tiles + (q < Q ? q : 0) * (r * T);
    const int ntiles = (d.w + T - 1) / T;
    for (int g0 = 0; g0 < ntiles; g0 += Q) {
        const bool on = q < Q && g0 + q < ntiles;
        const int v = d.v0 + (g0 + q) * T;          // the first column of the tile
        const int tw = min(T, d.v0 + d.w - v);      // its columns
        if (on) {
            for (int e = i0; e < r * T; e += step) {
                const int k = e / T, t = e - k * T;
                const i64d row = a.colmap ? a.colmap[d.brow + L.pivrow[k]] : d.brow + L.pivrow[k];
                tile[e] = t < tw ? zp_reduce(F, (int64_t)a.B[row * a.ldb + v + t]) : 0;
            }
            if (i0 == 0) bad[q] = 0;
        }
        __syncthreads();   // (the first round: perm too)
        int ypiv[T];
        if (on) {
            int mask = 0;
            for (int e = i0; e < m; e += step) {
                const int i = r > 0 ? perm[e] : e;
                int y[T];
                if (F.small) solver_dense_dot<true>(F, G + i * ldg, (const int4 *)tile, r, y);
                else solver_dense_dot<false>(F, G + i * ldg, (const int4 *)tile, r, y);
                if (e < r) {
#pragma unroll
                    for (int t = 0; t < T; t++) ypiv[t] = y[t];
                } else {
                    const i64d row = a.colmap ? a.colmap[d.brow + i] : d.brow + i;
                    const int *b = a.B + row * a.ldb + v;
#pragma unroll
                    for (int t = 0; t < T; t++)
                        if (t < tw && zp_add(F, y[t], zp_reduce(F, (int64_t)b[t])) != 0) mask |= 1 << t;
                }
            }
            if (mask) atomicOr(&bad[q], mask);
        }
        __syncthreads();
        if (on && i0 < r) {
#pragma unroll
            for (int t = 0; t < T; t++) tile[i0 * T + t] = ypiv[t];
        }
        __syncthreads();
        if (on) {
            const int nosol = bad[q];
            for (int j = i0; j < n; j += step) {
                int lo = 0, hi = r;   // the k with pivcol[k] == j, if any: pivcol ascends
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (L.pivcol[mid] < j) lo = mid + 1;
                    else hi = mid;
                }
                const bool piv = lo < r && L.pivcol[lo] == j;
                const i64d row = a.rowmap ? a.rowmap[d.xrow + j] : d.xrow + j;
                int *x = a.X + row * a.ldx + v;
#pragma unroll
                for (int t = 0; t < T; t++)
                    if (t < tw) x[t] = piv && !((nosol >> t) & 1) ? tile[lo * T + t] : 0;
            }
            if (i0 < tw) {
                if (a.flag) {
                    if ((nosol >> i0) & 1) atomicOr(a.flag + v + i0, 1u);
                } else a.ok[d.okoff + v + i0] = (nosol >> i0) & 1 ? 0 : 1;
            }
        }
        __syncthreads();
    }
}

// a blocks handle: block_cols[col_start[b] + col_pos[j]] = j, the global columns of every block in the block's order
__global__ void k_solver_block_cols(int m, const int *__restrict__ col_block, const int *__restrict__ col_pos, const i64d *__restrict__ col_start,
                                    int *__restrict__ block_cols)
{
    const i64d j = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m) block_cols[col_start[col_block[j]] + col_pos[j]] = (int)j;
}

// a blocks handle, after the blocks: ok[v] = no block failed on column v; a column that failed is zeroed in all n rows of X
__global__ void k_solver_dense_finish(int n, int K, const unsigned *__restrict__ flag, unsigned char *__restrict__ ok, int *__restrict__ X, i64d ldx)
{
    const i64d e = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    const i64d row = e / K;
    const int v = (int)(e - row * K);
    if (row >= (n > 0 ? n : 1)) return;
    const bool failed = flag[v] != 0;
    if (row == 0) ok[v] = failed ? 0 : 1;
    if (failed && row < n) X[row * ldx + v] = 0;
}
