// batch.hpp -- many small matrices echelonized in one launch: one workgroup per matrix, resident in LDS from first load to last store.
// The elimination itself (batch_eliminate) is shared with solve_batch.hpp.
//
// The whole batch is one concatenated device CSR (row pointers P as global entry offsets, columns J, values X) plus one
// descriptor per matrix.  A workgroup scatters its matrix into a dense n x m image of balanced residues (32-bit words, row
// stride ld), eliminates it with batch_eliminate over all m columns, so the image ends as the reduced row echelon form and the
// pivot columns are the canonical ones, and writes its output from the image.
//
// Row stride: the election and the factor pass walk DOWN a column, lane i at word i * ld + c.  ds_read_b32 / ds_write_b32 bank
// on (word mod 32) per half wave, so an odd ld makes the walk conflict-free and an even one folds it onto 32 / gcd(ld, 32) banks.
// ld = m for odd m, m + 1 for even m when the padded image still fits the largest class (BATCH_PAD_CAP), else m.
//
// Output of a workgroup, into its slices of the chunk's buffers (no atomics, no cross-workgroup traffic):
//   BATCH_LU      rec[0] = rank, rec[2 .. 2 + m) = qinv, rec[2 + m .. 2 + m + n) = p (elected rows in election order, then the
//                 others ascending); row k of U (k-th elected pivot = k-th pivot column) compacted in column order at
//                 scratch[slice + k * (m - r + 1)], its length in cnt[slot0 + k]
//   BATCH_KERNEL  rec[0] = rank; kernel vector t (t-th free column f) = {(pivcol(k), R[k][f])} in k order, then (f, -1), at
//                 scratch[slice + t * (r + 1)], its length in cnt[slot0 + t]
//   BATCH_RANK    rank[item] only (rows that are pivots already are not reduced further)
// k_batch_pack then copies the rows back to back at the exclusive scan of cnt, in the manner of k_spg_pack.
#pragma once
#include <hip/hip_runtime.h>
#include "zp.hpp"

#define BATCH_LIMIT 32768     // n * m <= this many words takes the LDS path (and n, m <= it)
#define BATCH_PAD_CAP 34816   // words of image the largest class holds: the limit + room for the padding of the stride
#define BATCH_NCLASS 4

enum { BATCH_LU = 0, BATCH_KERNEL = 1, BATCH_RANK = 2 };

struct BatchDesc {
    i64d row0;    // P[row0 .. row0 + n]: the row pointers of the matrix (offsets into J / X)
    i64d rec;     // its record in the chunk's output buffer (ints)
    i64d slice;   // its slice of the entry scratch (int2)
    i64d slot0;   // its first row slot in cnt
    int n, m, ld;
    int nslots;   // row slots: min(n, m) for BATCH_LU, m for BATCH_KERNEL
    ZpField F;
};

struct BatchArgs {
    const BatchDesc *desc;
    const int *items;          // descriptors of this launch (one class of one chunk)
    const i64d *P;
    const int *J;
    const int *X;
    int mode;
    int cap, bw, rmax;         // LDS layout of the class: image words, words per bitset, pivots
    int *rec;
    int2 *scratch;
    int *cnt;
    int *rank;                 // BATCH_RANK: indexed like desc
};

// words of LDS of a class besides the image: two bitsets (pivot rows, pivot columns), three pivot lists, the election's mailbox
__host__ __device__ inline int batch_lds_words(int cap, int bw, int rmax) { return cap + 2 * bw + 3 * rmax + 16; }

// the dynamic LDS of a class, carved in the order batch_lds_words counts it
struct BatchLds {
    int *img;
    unsigned *rowflag, *colflag;   // bit i: image row i is a pivot row / column i is a pivot column (colflag NULL: not kept)
    int *pivrow, *pivcol, *pinv;   // the k-th pivot: its image row, its column, the inverse of its entry
    int *wmin;                     // the election's mailbox: 2 parities x 8 waves
    __device__ BatchLds(int *base, int cap, int bw, int rmax, bool keep_colflag)
        : img(base), rowflag((unsigned *)(base + cap)), colflag(keep_colflag ? rowflag + bw : nullptr), pivrow((int *)(rowflag + 2 * bw)), pivcol(pivrow + rmax),
          pinv(pivcol + rmax), wmin(pinv + rmax)
    {
    }
};

// a zero image of `words` words and empty bitsets; the caller's barrier follows
template <int BS> __device__ inline void batch_lds_clear(const BatchLds &L, int words, int bw)
{
    for (int e = threadIdx.x; e < words; e += BS) L.img[e] = 0;
    for (int w = threadIdx.x; w < bw; w += BS) {
        L.rowflag[w] = 0;
        if (L.colflag) L.colflag[w] = 0;
    }
}

// How a workgroup of BS threads walks rows of `width` words: TX lanes per row (a power of two, at most a wave), TY rows at a time;
// this thread is lane tx of row ty
template <int BS> struct BatchLanes {
    int TX, tx, ty, TY;
    __device__ __forceinline__ explicit BatchLanes(int width)
    {
        int lt = 0;
        while ((1 << lt) < width && lt < 6) lt++;
        TX = 1 << lt, tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> lt, TY = BS >> lt;
    }
};

// Rows 0 .. n - 1 of a concatenated CSR (P = the row pointers of the matrix, J, X) into a cleared image of balanced residues:
// entry (i, j) at img[i * ld + j], TRANSPOSED at img[j * ld + i].  `width` = the most entries a row holds.  No barrier.
template <int BS, bool TRANSPOSED>
__device__ __forceinline__ void batch_load_rows(const ZpField &F, int *img, int ld, int n, int width, const i64d *P, const int *J, const int *X)
{
    const BatchLanes<BS> t(width);
    for (int i = t.ty; i < n; i += t.TY) {
        const i64d e0 = P[i], e1 = P[i + 1];
        for (i64d k = e0 + t.tx; k < e1; k += t.TX) img[TRANSPOSED ? J[k] * ld + i : i * ld + J[k]] = zp_reduce(F, (int64_t)X[k]);
    }
}

// Gauss-Jordan elimination of the image (`rows` rows of stride ld) inside LDS by the whole workgroup; returns the rank.  Columns
// 0 .. ecols - 1 are candidates for a pivot, in that order; the update reaches columns 0 .. ucols - 1 (ucols >= ecols: what lies
// right of the candidates rides along).  The rule is the one dense.hpp:5 states: the pivot of a column is the first row, not yet a
// pivot, that holds a non-zero there.  The pivot row is subtracted from EVERY other row that holds the column (earlier pivot rows
// too), so the candidate columns end in reduced row echelon form and the pivot columns are the canonical ones.
//
// Two shortcuts keep it to three barriers per pivot (one per block of BS rows the election scans, one after the factors, one
// after the update), both invisible in the result:
//   - pivot rows are not normalised in place: row pivrow[k] stays a multiple of its normalised form and the inverse of its pivot
//     is kept (pinv[k]); the factor of a row is f * pinv and whoever reads a pivot row multiplies by pinv once;
//   - column c is not zeroed: the factors are written over it (each row its own word) and read from there by the update.
//     Pivot columns of the final image therefore hold leftovers; nobody reads them (the pivot counts as 1).
// The election posts one candidate per wave into a mailbox and reads all of them after a barrier.  The mailbox has two halves
// used in turn (par): a wave that is still reading the one of this step cannot meet the writes of the next step, and the half of
// the step before last is free again because a barrier lies between.
//
// Once every row is a pivot no election can succeed, so the loop ends there.  skip_done_rows (wave-uniform): rows that are pivots
// already get the factor 0, which leaves the rank as it is and nothing else meaningful.  WITH_QINV: qinv[c] (global memory) = k for
// the k-th pivot's column c, -1 for a candidate column without pivot; without it qinv is not looked at.  (A template parameter
// because k_batch_elim needs 106 scalar registers with a run-time test of the pointer, which costs it the eighth wave per SIMD.)
template <int BS, bool WITH_QINV>
__device__ inline int batch_eliminate(const ZpField &F, const BatchLds &L, int ld, int rows, int ecols, int ucols, bool skip_done_rows, int *qinv)
{
    constexpr int NW = BS / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int *img = L.img, *wmin = L.wmin;
    unsigned *rowflag = L.rowflag;
    const BatchLanes<BS> t(ucols);   // the update
    const int TX = t.TX, tx = t.tx, ty = t.ty, TY = t.TY;

    int r = 0, par = 0, c = 0;
    for (; c < ecols && r < rows; c++) {
        // ---- election: the first row that is not a pivot yet and holds column c
        int pr = 0x7fffffff;
        for (int base = 0; base < rows; base += BS) {
            const int i = base + tid;
            const bool hit = i < rows && !((rowflag[i >> 5] >> (i & 31)) & 1u) && img[i * ld + c] != 0;
            const unsigned long long b = __ballot(hit);
            if (lane == 0) wmin[par * 8 + wave] = b ? base + wave * 64 + (__ffsll((long long)b) - 1) : 0x7fffffff;
            __syncthreads();
            int best = 0x7fffffff;
#pragma unroll
            for (int w = 0; w < NW; w++) best = min(best, wmin[par * 8 + w]);
            par ^= 1;
            if (best != 0x7fffffff) { pr = best; break; }
        }
        if (pr == 0x7fffffff) {
            if (WITH_QINV && tid == 0) qinv[c] = -1;
            continue;
        }
        const int inv = zp_inverse(F, img[pr * ld + c]);
        // ---- factors, in place on column c
        for (int i = tid; i < rows; i += BS) {
            if (i == pr) continue;
            const int f = img[i * ld + c];
            if (f == 0) continue;
            const bool done = skip_done_rows && ((rowflag[i >> 5] >> (i & 31)) & 1u);
            img[i * ld + c] = done ? 0 : zp_mul(F, f, inv);
        }
        __syncthreads();
        if (tid == 0) {
            rowflag[pr >> 5] |= 1u << (pr & 31);
            if (L.colflag) L.colflag[c >> 5] |= 1u << (c & 31);
            L.pivrow[r] = pr;
            L.pivcol[r] = c;
            L.pinv[r] = inv;
            if (WITH_QINV) qinv[c] = r;
        }
        // ---- update: row i -= factor * pivot row, on the columns right of c
        for (int i = ty; i < rows; i += TY) {
            if (i == pr) continue;
            const int g = img[i * ld + c];
            if (g == 0) continue;
            for (int j = c + 1 + tx; j < ucols; j += TX) {
                const int v = img[pr * ld + j];
                if (v != 0) img[i * ld + j] = zp_axpy(F, -g, v, img[i * ld + j]);
            }
        }
        __syncthreads();
        r++;
    }
    if (WITH_QINV)
        for (int k = c + tid; k < ecols; k += BS) qinv[k] = -1;
    return r;
}

// wave-level compaction: appends (j, v) of the lanes with v != 0 at dst[count ..], in lane order, and advances count (the same
// in every lane); the whole wave calls it
__device__ inline void batch_append(int2 *dst, int &count, int j, int v)
{
    const unsigned long long b = __ballot(v != 0);
    if (v != 0) dst[count + __popcll(b & ((1ull << (threadIdx.x & 63)) - 1ull))] = make_int2(j, v);
    count += __popcll(b);
}

template <int BS>
__global__ __launch_bounds__(BS) void k_batch_elim(BatchArgs a)
{
    extern __shared__ int s_batch[];
    constexpr int NW = BS / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int item = a.items[blockIdx.x];
    const BatchDesc d = a.desc[item];
    const ZpField F = d.F;
    const int n = d.n, m = d.m, ld = d.ld, mode = a.mode;
    const BatchLds L(s_batch, a.cap, a.bw, a.rmax, true);
    int *img = L.img, *pivrow = L.pivrow, *pivcol = L.pivcol, *pinv = L.pinv;
    unsigned *rowflag = L.rowflag, *colflag = L.colflag;

    batch_lds_clear<BS>(L, n * ld, a.bw);
    __syncthreads();
    batch_load_rows<BS, false>(F, img, ld, n, m, a.P + d.row0, a.J, a.X);
    __syncthreads();

    const int r = mode == BATCH_LU ? batch_eliminate<BS, true>(F, L, ld, n, m, m, false, a.rec + d.rec + 2)
                                   : batch_eliminate<BS, false>(F, L, ld, n, m, m, mode == BATCH_RANK, nullptr);

    if (mode == BATCH_RANK) {
        if (tid == 0) a.rank[item] = r;
        return;
    }
    int *rec = a.rec + d.rec;
    int *cnt = a.cnt + d.slot0;
    if (tid == 0) { rec[0] = r; rec[1] = 0; }
    if (mode == BATCH_LU) {
        const int stride = m - r + 1;
        for (int k = wave; k < r; k += NW) {
            const int pr = pivrow[k], pc = pivcol[k], inv = pinv[k];
            int2 *dst = a.scratch + d.slice + (i64d)k * stride;
            int count = 0;
            for (int j0 = pc; j0 < m; j0 += 64) {
                const int j = j0 + lane;
                int v = 0;
                if (j == pc) v = 1;
                else if (j < m && !((colflag[j >> 5] >> (j & 31)) & 1u)) {
                    const int x = img[pr * ld + j];
                    if (x != 0) v = zp_mul(F, x, inv);
                }
                batch_append(dst, count, j, v);
            }
            if (lane == 0) cnt[k] = count;
        }
        for (int k = r + tid; k < d.nslots; k += BS) cnt[k] = 0;
        __syncthreads();
        // p: the elected rows, then the others ascending (their places from the popcounts of the words before them)
        int *woff = (int *)colflag;
        if (tid == 0) {
            int off = 0;
            for (int w = 0; w * 32 < n; w++) { woff[w] = off; off += __popc(~rowflag[w]); }
        }
        __syncthreads();
        int *p = rec + 2 + m;
        for (int k = tid; k < r; k += BS) p[k] = pivrow[k];
        for (int i = tid; i < n; i += BS) {
            const unsigned free_rows = ~rowflag[i >> 5];
            if ((free_rows >> (i & 31)) & 1u) p[r + woff[i >> 5] + __popc(free_rows & ((1u << (i & 31)) - 1u))] = i;
        }
    } else {
        const int stride = r + 1;
        int *woff = (int *)rowflag;
        __syncthreads();
        if (tid == 0) {
            int off = 0;
            for (int w = 0; w * 32 < m; w++) { woff[w] = off; off += __popc(colflag[w]); }
        }
        __syncthreads();
        for (int f = wave; f < m; f += NW) {
            const unsigned word = colflag[f >> 5];
            if ((word >> (f & 31)) & 1u) continue;
            const int t = f - (woff[f >> 5] + __popc(word & ((1u << (f & 31)) - 1u)));
            int2 *dst = a.scratch + d.slice + (i64d)t * stride;
            int count = 0;
            for (int k0 = 0; k0 < r; k0 += 64) {
                const int k = k0 + lane;
                int v = 0, pc = 0;
                if (k < r) {
                    pc = pivcol[k];
                    if (pc < f) {
                        const int x = img[pivrow[k] * ld + f];
                        if (x != 0) v = zp_mul(F, x, pinv[k]);
                    }
                }
                batch_append(dst, count, pc, v);
            }
            if (lane == 0) {
                dst[count] = make_int2(f, -1);
                cnt[t] = count + 1;
            }
        }
        for (int t = m - r + tid; t < d.nslots; t += BS) cnt[t] = 0;
    }
}

// the rows of a chunk back to back: one wave per matrix, row k of its slice to out[rowstart[slot0 + k] ..]
__global__ __launch_bounds__(64) void k_batch_pack(const BatchDesc *__restrict__ desc, const int *__restrict__ items, int mode, const int *__restrict__ rec,
                                                   const int *__restrict__ cnt, const i64d *__restrict__ rowstart, const int2 *__restrict__ scratch,
                                                   int2 *__restrict__ out)
{
    const BatchDesc d = desc[items[blockIdx.x]];
    const int r = rec[d.rec];
    const int rows = mode == BATCH_LU ? r : d.m - r;
    const int stride = mode == BATCH_LU ? d.m - r + 1 : r + 1;
    for (int k = 0; k < rows; k++) {
        const int c = cnt[d.slot0 + k];
        const int2 *src = scratch + d.slice + (i64d)k * stride;
        int2 *dst = out + rowstart[d.slot0 + k];
        for (int e = threadIdx.x; e < c; e += 64) dst[e] = src[e];
    }
}
