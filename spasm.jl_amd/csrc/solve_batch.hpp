// solve_batch.hpp -- X * A = B for many small matrices in one launch: one workgroup per (matrix, slab of right-hand sides), resident
// in LDS from first load to last store.  The companion of batch.hpp; it shares that file's limits, classes, LDS layout and
// elimination (batch_eliminate, which states the election rule and what the image holds afterwards).
//
// x * A = b is A^T * x^T = b^T.  A workgroup scatters the TRANSPOSED, AUGMENTED image into LDS: m rows (the columns of A), n + w
// columns (the n rows of A, then the w right-hand sides of its slab, one per column), balanced residues in 32-bit words, row stride
// ld.  It eliminates the image with the first n columns as candidates; the right-hand-side columns lie right of every candidate,
// so they ride along in the update.
//
// Column c of the image is row c of A, and a column is elected exactly when it is not a combination of the columns before it.  The
// pivot columns are therefore the CANONICAL ROW BASIS of A: row j belongs to it iff it is not a combination of rows 0 .. j-1.  After
// the elimination the pivot rows hold a multiple of the identity on the pivot columns, so for right-hand side t
//   ok      iff every image row that is not a pivot row holds a zero in column n + t
//   x[c_k]  = img[pr_k][n + t] * pinv[k] for the k-th pivot (image row pr_k, column c_k), every other x[i] = 0:
// the unique solution that is zero outside the canonical basis.  c_k ascends with k, so a row of X comes out in column order.
// Nothing here depends on which right-hand sides share a slab: a column of the image is never read by the update of another one.
//
// Row stride.  The election, the factor pass and the ok test walk DOWN a column (lane i at word i * ld + c); as in batch.hpp an odd
// ld makes that walk conflict-free over the 32 banks a half wave sees and an even one folds it onto 32 / gcd(ld, 32) of them.  ld =
// n + w when that is odd, n + w + 1 when the padded image still fits the class; a slab that is one of several gives up a column
// instead (w - 1), so only a single slab that fills its class to the last word runs on an even stride.
//
// Output of a workgroup (no atomics, every word has one writer): for its right-hand side t, slot = slot0 + t:
//   ok[slot], cnt[slot] = entries of the row of X (0 when there is no solution), src[slot] = where they start in the entry scratch
//   (slice + t * (r + 1)), the entries (c_k, x[c_k]) with x[c_k] != 0 in k order.
// k_solve_pack then copies the rows back to back at the exclusive scan of cnt.
//
// The second half of the file splits a right-hand side over the blocks of a spasm_amd_blocks handle and puts the blocks' solutions
// back together, all on the device (spasm_amd_blocks_solve in engine.hip states the pipeline).
#pragma once
#include <hip/hip_runtime.h>
#include "batch.hpp"

struct SolveDesc {
    i64d row0;    // P[row0 .. row0 + n]: the row pointers of A
    i64d brow0;   // BP[brow0 .. brow0 + w]: the row pointers of the right-hand sides of this slab
    i64d slice;   // its slice of the entry scratch (int2): w * (min(n, m) + 1)
    i64d slot0;   // the slot of its first right-hand side in ok / cnt / src
    int n, m, w, ld;
    ZpField F;
};

struct SolveBatchArgs {
    const SolveDesc *desc;
    const int *items;          // descriptors of this launch (one class)
    const i64d *P;             // A: concatenated CSR
    const int *J;
    const int *X;
    const i64d *BP;            // right-hand sides: concatenated CSR
    const int *BJ;
    const int *BX;
    int cap, bw, rmax;         // LDS layout of the class, as in BatchArgs
    int2 *scratch;
    int *cnt;
    i64d *src;
    unsigned char *ok;
};

template <int BS>
__global__ __launch_bounds__(BS) void k_solve_elim(SolveBatchArgs a)
{
    extern __shared__ int s_solve[];
    constexpr int NW = BS / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SolveDesc d = a.desc[a.items[blockIdx.x]];
    const ZpField F = d.F;
    const int n = d.n, m = d.m, ld = d.ld, W = d.n + d.w;
    const BatchLds L(s_solve, a.cap, a.bw, a.rmax, false); // (the pivot columns are not asked for)
    int *img = L.img;

    batch_lds_clear<BS>(L, m * ld, a.bw);
    __syncthreads();
    {
        // A and B in one loop (the transposed twin of batch_load_rows with a select per row); a row of either holds at most m entries
        const BatchLanes<BS> t(m);
        const int TX = t.TX, tx = t.tx, ty = t.ty, TY = t.TY;
        for (int i = ty; i < W; i += TY) {
            const bool rhs = i >= n;
            const i64d e0 = rhs ? a.BP[d.brow0 + (i - n)] : a.P[d.row0 + i], e1 = rhs ? a.BP[d.brow0 + (i - n) + 1] : a.P[d.row0 + i + 1];
            const int *cj = rhs ? a.BJ : a.J, *cx = rhs ? a.BX : a.X;
            for (i64d k = e0 + tx; k < e1; k += TX) img[cj[k] * ld + i] = zp_reduce(F, (int64_t)cx[k]);
        }
    }
    __syncthreads();

    const int r = batch_eliminate<BS, false>(F, L, ld, m, n, W, false, nullptr);

    // ---- one wave per right-hand side: the test down its column, then its row of X
    for (int t = wave; t < d.w; t += NW) {
        const int col = n + t;
        bool bad = false;
        for (int i0 = 0; i0 < m && !bad; i0 += 64) {
            const int i = i0 + lane;
            const bool hit = i < m && !((L.rowflag[i >> 5] >> (i & 31)) & 1u) && img[i * ld + col] != 0;
            bad = __ballot(hit) != 0ull;
        }
        const i64d at = d.slice + (i64d)t * (r + 1);
        int2 *dst = a.scratch + at;
        int count = 0;
        for (int k0 = 0; k0 < r && !bad; k0 += 64) {
            const int k = k0 + lane;
            int v = 0, pc = 0;
            if (k < r) {
                pc = L.pivcol[k];
                const int x = img[L.pivrow[k] * ld + col];
                if (x != 0) v = zp_mul(F, x, L.pinv[k]);
            }
            batch_append(dst, count, pc, v);
        }
        if (lane == 0) {
            a.cnt[d.slot0 + t] = count;
            a.src[d.slot0 + t] = at;
            a.ok[d.slot0 + t] = bad ? 0 : 1;
        }
    }
}

// the rows of a chunk back to back: one wave per slot
__global__ __launch_bounds__(64) void k_solve_pack(const int *__restrict__ cnt, const i64d *__restrict__ src, const i64d *__restrict__ rowstart,
                                                   const int2 *__restrict__ scratch, int2 *__restrict__ out)
{
    const i64d slot = blockIdx.x;
    const int c = cnt[slot];
    const int2 *from = scratch + src[slot];
    int2 *dst = out + rowstart[slot];
    for (int e = threadIdx.x; e < c; e += 64) dst[e] = from[e];
}

// ------------------------------------------------------------------------------------------------
// A right-hand side over the blocks of a handle.  An entry (k, j) of Rhs belongs to block col_block[j]; the entries sorted (stable)
// by (block, k) fall into RUNS of one key each, and run q IS the right-hand side "row k of Rhs restricted to the columns of block b".
// The runs of a block are consecutive and ascend in k, so run_start is the row-pointer array of all blocks' right-hand sides at once
// and the run number is the slot k_solve_elim writes to.
// ------------------------------------------------------------------------------------------------

// key = block << 32 | row of the entry (found by bisection in the row pointers), value = the entry
__global__ void k_sv_keys(int K, i64d e0, i64d ne, const i64d *__restrict__ rp, const int *__restrict__ rj, const int *__restrict__ col_block,
                          unsigned long long *__restrict__ key, int *__restrict__ val)
{
    const i64d q = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= ne) return;
    const i64d e = e0 + q;
    int lo = 0, hi = K; // the last row with rp[row] <= e (rp[lo] <= e < rp[hi] throughout)
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (rp[mid] <= e) lo = mid;
        else hi = mid;
    }
    key[q] = ((unsigned long long)(unsigned)col_block[rj[e]] << 32) | (unsigned)lo;
    val[q] = (int)q;
}

__global__ void k_sv_heads(i64d ne, const unsigned long long *__restrict__ key, int *__restrict__ head)
{
    const i64d q = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    if (q > ne) return;
    head[q] = q < ne && (q == 0 || key[q] != key[q - 1]) ? 1 : 0;
}

// the runs (start, block, row) and the sorted entries in block coordinates; run_start[nruns] = ne
__global__ void k_sv_runs(i64d e0, i64d ne, const unsigned long long *__restrict__ key, const int *__restrict__ val, const int *__restrict__ head,
                          const int *__restrict__ runid, const int *__restrict__ rj, const int *__restrict__ rx, const int *__restrict__ col_pos,
                          i64d *__restrict__ run_start, int *__restrict__ run_block, int *__restrict__ run_row, int *__restrict__ sj, int *__restrict__ sx)
{
    const i64d q = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    if (q > ne) return;
    if (q == ne) { run_start[runid[ne]] = ne; return; }
    const i64d e = e0 + val[q];
    sj[q] = col_pos[rj[e]];
    sx[q] = rx[e];
    if (head[q]) {
        const int id = runid[q];
        run_start[id] = q;
        run_block[id] = (int)(key[q] >> 32);
        run_row[id] = (int)(key[q] & 0xffffffffu);
    }
}

// every slot starts as "solved by the empty row"; the run of a block without rows (an empty column of A) is solvable iff its
// entries vanish mod p
__global__ void k_sv_init(int nruns, ZpField F, const i64d *__restrict__ run_start, const int *__restrict__ run_block, const i64d *__restrict__ row_start,
                          const int *__restrict__ sx, int *__restrict__ cnt, i64d *__restrict__ src, unsigned char *__restrict__ ok, int *__restrict__ iota)
{
    const i64d q = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nruns) return;
    const int b = run_block[q];
    bool good = true;
    if (row_start[b + 1] == row_start[b])
        for (i64d e = run_start[q]; e < run_start[q + 1]; e++) good = good && zp_reduce(F, (int64_t)sx[e]) == 0;
    cnt[q] = 0;
    src[q] = 0;
    ok[q] = good ? 1 : 0;
    iota[q] = (int)q;
}

// rows of Rhs: ok[k] = AND over the runs of row k (byrow = the runs sorted by row, krun = where the runs of a row start); a run of
// a row without solution contributes nothing
__global__ void k_sv_rowok(int K, const i64d *__restrict__ krun, const int *__restrict__ byrow, const unsigned char *__restrict__ ok, const int *__restrict__ cnt,
                           unsigned char *__restrict__ rowok, int *__restrict__ len)
{
    const i64d k = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    bool good = true;
    for (i64d q = krun[k]; q < krun[k + 1]; q++) good = good && ok[byrow[q]];
    rowok[k] = good ? 1 : 0;
    for (i64d q = krun[k]; q < krun[k + 1]; q++) len[byrow[q]] = good ? cnt[byrow[q]] : 0;
}

// the entries of a run as (row << 32 | row of A, value): one wave per run
__global__ __launch_bounds__(64) void k_sv_emit(const int *__restrict__ len, const i64d *__restrict__ off, const i64d *__restrict__ src, const int *__restrict__ run_block,
                                                const int *__restrict__ run_row, const i64d *__restrict__ row_start, const int *__restrict__ block_rows,
                                                const int2 *__restrict__ scratch, unsigned long long *__restrict__ key, int *__restrict__ val)
{
    const i64d q = blockIdx.x;
    const int c = len[q];
    const int2 *from = scratch + src[q];
    const int *rows = block_rows + row_start[run_block[q]];
    const unsigned long long hi = (unsigned long long)(unsigned)run_row[q] << 32;
    for (int e = threadIdx.x; e < c; e += 64) {
        const int2 v = from[e];
        key[off[q] + e] = hi | (unsigned)rows[v.x];
        val[off[q] + e] = v.y;
    }
}

// row pointers of X from the sorted keys (p[k] = first place with a key of row >= k), and its columns
__global__ void k_sv_finish(int K, i64d total, const unsigned long long *__restrict__ key, i64d *__restrict__ p, int *__restrict__ j)
{
    const i64d t = (i64d)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < total) j[t] = (int)(key[t] & 0xffffffffu);
    if (t > K) return;
    const unsigned long long want = (unsigned long long)t << 32;
    i64d lo = 0, hi = total;
    while (lo < hi) {
        const i64d mid = lo + (hi - lo) / 2;
        if (key[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    p[t] = lo;
}
